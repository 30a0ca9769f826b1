// lbm_reduce.hpp -- the one reduction tree of the samplers (monitor, residual, topology), written over an accumulator type A:
//   static A identity()                  what a lane starts from
//   static void fold(A& a, const A& b)   a := a (+) b, the one combining step of every level (sums: a + b in this order)
//   void each(f)                         f(member&) for the members in order: the order of a stored accumulator's doubles
//   static constexpr int VALS            the number of members
// The order of combination is fixed, so a result depends on the lattice and the grid alone: a lane folds its cells in grid-stride
// order; the lanes of a wave combine by shuffles with offsets 32, 16, .., 1, fold(a, value of lane + off); lane 0 of each wave
// stores to LDS and thread 0 folds waves 1, 2, .. in index order into one partial result per workgroup; the final pass is one wave,
// lane l folds the partial results l * chunk .. (l + 1) * chunk - 1 in index order and the same shuffle tree follows.  No atomics.
// int members travel through the shuffles as int and through memory as doubles.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

constexpr int RED_WAVE = 64;

// wave-64 tree through shuffles: lane 0 ends with the wave's result
template <typename A>
__device__ __forceinline__ void red_wave(A& a) {
#pragma unroll
    for (int off = RED_WAVE / 2; off > 0; off >>= 1) {
        A b = a;
        b.each([&](auto& m) { m = __shfl_down(m, off, RED_WAVE); });
        A::fold(a, b);
    }
}

template <typename A>
__device__ __forceinline__ void red_store(double* __restrict__ p, A a) {
    int i = 0;
    a.each([&](auto& m) { p[i++] = (double)m; });
}
template <typename A>
__device__ __forceinline__ A red_load(const double* __restrict__ p) {
    A a = A::identity();
    int i = 0;
    a.each([&](auto& m) { m = (std::remove_reference_t<decltype(m)>)p[i++]; });
    return a;
}

// The workgroup's waves (each reduced by red_wave already) through sh: true for thread 0, whose a is then the workgroup's result.
template <typename A, int WAVES>
__device__ __forceinline__ bool red_workgroup(A& a, double (*sh)[A::VALS]) {
    if (threadIdx.x % RED_WAVE == 0) red_store(sh[threadIdx.x / RED_WAVE], a);
    __syncthreads();
    if (threadIdx.x != 0) return false;
    for (int w = 1; w < WAVES; ++w) A::fold(a, red_load<A>(sh[w]));
    return true;
}

// The final pass of one wave over nper partial results: lane 0 returns the result.
template <typename A>
__device__ __forceinline__ A red_final(const double* __restrict__ partial, int nper) {
    const int lane = threadIdx.x, chunk = (nper + RED_WAVE - 1) / RED_WAVE;
    A a = A::identity();
    for (int i = lane * chunk; i < nper && i < (lane + 1) * chunk; ++i) A::fold(a, red_load<A>(partial + (size_t)i * A::VALS));
    red_wave(a);
    return a;
}
