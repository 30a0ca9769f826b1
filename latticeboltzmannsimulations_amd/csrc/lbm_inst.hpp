// lbm_inst.hpp -- the explicit instantiations of the multi-step kernels: one list of the operator variants that dispatch() (lbm_host.hpp)
// can produce, and one line per kernel family over it.  The host units see `extern` declarations of every family for both real types.
// An instantiation unit lbm_<family>_<real>.hip defines LBM_INST as its family's line for its real type (e.g. LBM_INST_STREAMW(float))
// and holds those definitions alone: one unit per family and real type, compiled in parallel.
#pragma once
#include "lbm_stream.hpp"

// (real, collision operator, semantics, Smagorinsky) -- MRT_GPU.py semantics: six collision variants, with and without the closure
#define LBM_GPU_VARIANTS(M, R)                                                                                                  \
    M(R, C_SRT, SEM_GPU, false) M(R, C_TRT, SEM_GPU, false) M(R, C_MRT, SEM_GPU, false)                                         \
    M(R, C_MRT_FAST, SEM_GPU, false) M(R, C_SRT_FAST, SEM_GPU, false) M(R, C_TRT_FAST, SEM_GPU, false)                          \
    M(R, C_SRT, SEM_GPU, true) M(R, C_TRT, SEM_GPU, true) M(R, C_MRT, SEM_GPU, true)                                            \
    M(R, C_MRT_FAST, SEM_GPU, true) M(R, C_SRT_FAST, SEM_GPU, true) M(R, C_TRT_FAST, SEM_GPU, true)
// ... MRT.py semantics: the three strict ones
#define LBM_PY_VARIANTS(M, R) M(R, C_SRT, SEM_PY, false) M(R, C_TRT, SEM_PY, false) M(R, C_MRT, SEM_PY, false)
// ... half-way bounce-back: the three strict operators and the three fast ones, no closure (validate_params)
#define LBM_BB_VARIANTS(M, R)                                                                                                   \
    M(R, C_SRT, SEM_BB, false) M(R, C_TRT, SEM_BB, false) M(R, C_MRT, SEM_BB, false)                                            \
    M(R, C_MRT_FAST, SEM_BB, false) M(R, C_SRT_FAST, SEM_BB, false) M(R, C_TRT_FAST, SEM_BB, false)
// ... arith = promoted (float only: fp64 runs the strict variants), MRT_GPU.py semantics: the three promoted operators, with and without the closure
#define LBM_PROM_VARIANTS(M, R)                                                                                                 \
    M(R, C_SRT_PROM, SEM_GPU, false) M(R, C_TRT_PROM, SEM_GPU, false) M(R, C_MRT_PROM, SEM_GPU, false)                          \
    M(R, C_SRT_PROM, SEM_GPU, true) M(R, C_TRT_PROM, SEM_GPU, true) M(R, C_MRT_PROM, SEM_GPU, true)

// one instantiation of each kernel (LBM_X: `extern`, or nothing in the unit that compiles it)
#define LBM_TILE_ONE(R, COLL, SEM, S, TURB)                                                                                     \
    LBM_X template __global__ void k_stepS_deep<R, COLL, SEM, S, false, TURB>(const R* __restrict__, R* __restrict__, Geo, Relax<R>, Batch<R>, \
                                                                              int, int, int, int, int, FramePtrs<R>, int, int, int, int, int);
#define LBM_TILE_S(R, COLL, SEM, TURB) LBM_TILE_ONE(R, COLL, SEM, 3, TURB) LBM_TILE_ONE(R, COLL, SEM, 4, TURB) LBM_TILE_ONE(R, COLL, SEM, 5, TURB)
#define LBM_STREAM_ONE(R, COLL, SEM, TURB)                                                                                      \
    LBM_X template __global__ void k_stream<R, COLL, SEM, TURB>(const R* __restrict__, R* __restrict__, Geo, Relax<R>, int, int, int, int, int, \
                                                                int, FramePtrs<R>, int, int, int, int, int, int, int, int, int);
#define LBM_STREAMW_ONE(R, COLL, SEM, TURB) \
    LBM_X template __global__ void k_stream_walls<R, COLL, TURB>(const R* __restrict__, R* __restrict__, Geo, Relax<R>, int, int, int, int);
#define LBM_STREAMS_ONE(R, COLL, SEM, TURB)                                                                                     \
    LBM_X template __global__ void k_stream_walls_slab<R, COLL, TURB>(const R* __restrict__, R* __restrict__, Geo, Relax<R>, int, int, int, int, \
                                                                      int, int, int, int, int, int);
#define LBM_STREAMP_ONE(R, COLL, SEM, TURB) \
    LBM_X template __global__ void k_stream_pairs<R, COLL, TURB>(const R* __restrict__, R* __restrict__, Geo, Relax<R>, int, int, int, int);

// the families: the tile kernel (S = 3 .. 5 steps per launch) and k_stream in both semantics, the kernels with the walls inside
// (k_stream_walls, k_stream_walls_slab, k_stream_pairs) in MRT_GPU.py semantics
#define LBM_INST_TILES(R) LBM_GPU_VARIANTS(LBM_TILE_S, R) LBM_PY_VARIANTS(LBM_TILE_S, R)
#define LBM_INST_STREAM(R) LBM_GPU_VARIANTS(LBM_STREAM_ONE, R) LBM_PY_VARIANTS(LBM_STREAM_ONE, R)
#define LBM_INST_STREAMW(R) LBM_GPU_VARIANTS(LBM_STREAMW_ONE, R)
#define LBM_INST_STREAMS(R) LBM_GPU_VARIANTS(LBM_STREAMS_ONE, R)
#define LBM_INST_STREAMP(R) LBM_GPU_VARIANTS(LBM_STREAMP_ONE, R)
// the promoted operators in every family but k_stream_pairs (plan_kernel refuses stream_pairs with arith = promoted), in two units of their own
#define LBM_INST_TILES_PROM(R) LBM_PROM_VARIANTS(LBM_TILE_S, R)
#define LBM_INST_STREAM_PROM(R) LBM_PROM_VARIANTS(LBM_STREAM_ONE, R) LBM_PROM_VARIANTS(LBM_STREAMW_ONE, R) LBM_PROM_VARIANTS(LBM_STREAMS_ONE, R)
// bounce-back walls in the tile kernel and in k_stream (the frame workgroups of both run the wall rules; the walls-inside kernels refuse
// the semantics), in units of their own.  The tiles and the streaming segments themselves never compute a perimeter cell.
#define LBM_INST_TILES_BB(R) LBM_BB_VARIANTS(LBM_TILE_S, R)
#define LBM_INST_STREAM_BB(R) LBM_BB_VARIANTS(LBM_STREAM_ONE, R)
// ... and with solid cells inside the bounce-back cavity (LBM_FLAG_SOLID_TILES): the tile kernel over the same six operators, in units
// of its own (update_tile_inplace's SOLID path; the frame workgroups run gather_a's solid rule)
#define LBM_SOLID_VARIANTS(M, R)                                                                                                \
    M(R, C_SRT, SEM_SOLID, false) M(R, C_TRT, SEM_SOLID, false) M(R, C_MRT, SEM_SOLID, false)                                   \
    M(R, C_MRT_FAST, SEM_SOLID, false) M(R, C_SRT_FAST, SEM_SOLID, false) M(R, C_TRT_FAST, SEM_SOLID, false)
#define LBM_INST_TILES_SOLID(R) LBM_SOLID_VARIANTS(LBM_TILE_S, R)

#ifdef LBM_INST
#define LBM_X
LBM_INST
#else
#define LBM_X extern
LBM_INST_TILES(float) LBM_INST_TILES(double)
LBM_INST_STREAM(float) LBM_INST_STREAM(double)
LBM_INST_STREAMW(float) LBM_INST_STREAMW(double)
LBM_INST_STREAMS(float) LBM_INST_STREAMS(double)
LBM_INST_STREAMP(float) LBM_INST_STREAMP(double)
LBM_INST_TILES_PROM(float) LBM_INST_STREAM_PROM(float)
LBM_INST_TILES_BB(float) LBM_INST_TILES_BB(double)
LBM_INST_STREAM_BB(float) LBM_INST_STREAM_BB(double)
LBM_INST_TILES_SOLID(float) LBM_INST_TILES_SOLID(double)
#endif
