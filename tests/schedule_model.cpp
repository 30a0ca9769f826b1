// schedule_model.cpp -- a model of the step loop over the library's sampling schedule (csrc/lbm_schedule.hpp), for
// tests/test_schedule_cpu.py: "sample whatever is due, then advance by min(Smax, steps to the cut, steps left)", as step_many and
// sample_if_due do.  For every combination of `every` of the three samplers and every Smax it prints one run:
//   run e0 e1 e2 Smax / arm i nsteps / sample i n nsteps / unit from to / end
// The samplers are armed at step counts 0, 4 and 7 (the run steps there first), then come calls of 5, 20, 1 and 13 steps.
#include <cstdio>

#include "lbm_schedule.hpp"

using namespace lbmhost;

static Sampler sampler[NSAMPLERS];
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
    }
}

int main() {
    const int every[] = {0, 1, 3, 4, 5, 8, 13}, smax[] = {1, 5, 8, 10}, begin[NSAMPLERS] = {0, 4, 7}, calls[] = {5, 20, 1, 13};
    for (int e0 : every)
        for (int e1 : every)
            for (int e2 : every)
                for (int sm : smax) {
                    const int e[NSAMPLERS] = {e0, e1, e2};
                    std::printf("run %d %d %d %d\n", e0, e1, e2, sm);
                    nsteps = 0;
                    for (Sampler& s : sampler) s.clear();
                    for (int i = 0; i < NSAMPLERS; ++i) {
                        step((int)(begin[i] - nsteps), sm);
                        sampler[i].arm(nsteps, e[i]);
                        std::printf("arm %d %lld\n", i, nsteps);
                        const char* stem = automatic_sampler(sampler);
                        std::printf("automatic %s\n", stem ? stem : "-");
                    }
                    for (int n : calls) step(n, sm);
                    std::printf("end %lld\n", nsteps);
                }
    return 0;
}
