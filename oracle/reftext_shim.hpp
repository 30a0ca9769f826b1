/* Host shim for the CUDA kernel text that oracle/reftext.py extracts from the reference's MRT_GPU.py.  TEST INFRASTRUCTURE ONLY.
 *
 * The text is straight-line per-thread code: no barrier, its two __shared__ arrays receive the same constants from every
 * thread before use, and a thread reads only its own cell (the one cross-cell read feeds a value that the next line overwrites).
 * So it compiles as host C++ once the CUDA names below exist, and reftext_driver.inc may call it for the threads of a launch in
 * any order.  Nothing of the text itself is in this file. */
#pragma once
#include <cmath>
#include <cstdlib>
#include <type_traits>

#define __global__ static
#define __shared__ static

struct reftext_uint3 { unsigned int x, y, z; };              /* CUDA's uint3 / dim3: the members are unsigned */
static reftext_uint3 threadIdx, blockIdx, blockDim, gridDim;

static inline int min(int a, int b) { return a < b ? a : b; }

/* nvcc resolves abs / sqrt / exp of a float to the float overload; plain C's abs(int) would truncate the momentum flux */
using std::abs;
using std::exp;
using std::sqrt;
static_assert(std::is_same<decltype(abs(1.0f)), float>::value, "abs(float) must be the floating overload");
static_assert(std::is_same<decltype(sqrt(1.0f)), float>::value, "sqrt(float) must be the float overload");
static_assert(std::is_same<decltype(exp(1.0f)), float>::value, "exp(float) must be the float overload");
static_assert(std::is_same<decltype(sqrt(1.0)), double>::value, "sqrt(double) must stay double");
