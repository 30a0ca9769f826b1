// force_schedule_model.cpp -- a model of the step loop over the library's sampling schedule (csrc/lbm_schedule.hpp) with the force
// sampler in it, for tests/test_body_force_cpu.py: "take the field samples that are due, advance by min(Smax, steps to the cut, steps
// left), take the force sample that is due", as step_many does with sample_if_due and sample_after_unit.  For every pair of `every` of
// the residual (a field sampler: its sample of n reads the lattice after n - 1 steps) and of the force (after n steps) and every Smax it
// prints one run:
//   run e_residual e_force Smax / arm i nsteps / automatic stem / sample i n nsteps / unit from to / return nsteps / end
// The residual is armed at step count 2 and the force at 3 (the run steps there first), then come calls of 5, 20, 1 and 13 steps.
#include <cstdio>

#include "lbm_schedule.hpp"

using namespace lbmhost;

static Sampler sampler[NSCHEDULED];
static long long nsteps;

static void step(int n, int smax) {
    long long left = n;
    while (left > 0) {
        for (int i = 0; i < NSAMPLERS; ++i)
            if (sampler[i].due(nsteps)) {
                std::printf("sample %d %lld %lld\n", i, sampler[i].next, nsteps);
                sampler[i].advance();
            }
        long long S = steps_to_cut(sampler, nsteps, left);
        if (S > smax) S = smax;
        std::printf("unit %lld %lld\n", nsteps, nsteps + S);
        nsteps += S;
        left -= S;
        if (sampler[SMP_FORCE].due(nsteps)) {
            std::printf("sample %d %lld %lld\n", (int)SMP_FORCE, sampler[SMP_FORCE].next, nsteps);
            sampler[SMP_FORCE].advance();
        }
    }
    std::printf("return %lld\n", nsteps);
}

int main() {
    const int every[] = {0, 1, 3, 4, 5, 7, 8, 13}, smax[] = {1, 5, 8}, calls[] = {5, 20, 1, 13};
    for (int er : every)
        for (int ef : every)
            for (int sm : smax) {
                std::printf("run %d %d %d\n", er, ef, sm);
                nsteps = 0;
                for (Sampler& s : sampler) s.clear();
                step(2, sm);
                sampler[SMP_RESIDUAL].arm(nsteps, er);
                std::printf("arm %d %lld\n", (int)SMP_RESIDUAL, nsteps);
                step(1, sm);
                sampler[SMP_FORCE].arm(nsteps, ef, 1);
                std::printf("arm %d %lld\n", (int)SMP_FORCE, nsteps);
                const char* stem = automatic_sampler(sampler);
                std::printf("automatic %s\n", stem ? stem : "-");
                for (int n : calls) step(n, sm);
                std::printf("end %lld\n", nsteps);
            }
    return 0;
}
