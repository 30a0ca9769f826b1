// lbm_solid_move.hpp -- the step kernels of a lattice whose solid bodies move (lbm_set_body_motion; contract in include/lbm.h, DESIGN.md
// 2.10): k_step_solid and k_step_generic<.., SEM_SOLID> with the store-side add of Ladd's term compiled in (the MOVE block below, and
// MOVE of update_cell_a, lbm_device.hpp).  Launched only while a nonzero motion is set; a context at rest launches the
// kernels it always did.  Instantiated in lbm_solid_move_f32.hip / lbm_solid_move_f64.hip, units of their own, so that the units of
// k_step_solid, k_step_generic and the tile kernel keep their text.
#pragma once
#include "lbm_solid.hpp"

// cell_row[batch][ny][nx] (x fastest; -1, or the cell's row of delta), delta[rows][8] in the lattice type: lbm_wall_motion.hpp.
//
// k_step_solid (lbm_solid.hpp) line for line, plus the block marked MOVE between the collision and the pinning of the solid lanes.  It is
// a kernel of its own and not a switch of k_step_solid's body: a shared body, however it is inlined, changes the register allocation of
// the kernel at rest, whose text stays what it was.  The two are held together by the tests, which compare each route
// with the CPU reference bit for bit.
template <typename R, int COLL, bool NT>
__global__ __launch_bounds__(BLK) void k_step_solid_move(const R* __restrict__ src, R* __restrict__ dst, Geo geo, Relax<R> w, Batch<R> bt, int raw,
                                                         int row0, int row_stride, int nxb, int nblocks, const int32_t* __restrict__ cell_row,
                                                         const R* __restrict__ delta) {
    constexpr int V = 16 / (int)sizeof(R);
    typedef typename VecT<R, V>::type T;
    LBM_BATCH_SELECT(blockIdx.y)
    const int b = xcd_band(blockIdx.x, nblocks);
    const int y = row0 + (b / nxb) * row_stride, gy = geo.y0 + y;
    const int x0 = ((b % nxb) * BLK + threadIdx.x) * V;
    if (x0 >= geo.nx) return;
    const long long me = geo.at(x0, y);
    const T lk = vload<R, V, NT>(src + K_LINK * geo.plane + me, true);
    int lw[V], any = 0;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        lw[c] = (int)lk[c];
        any |= lw[c];
    }
    T in[Q], outv[Q], hq, hr;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        const int cx = raw ? 0 : cxk(k), cy = raw ? 0 : cyk(k);
        in[k] = vload<R, V, NT>(src + k * geo.plane + geo.at(x0 - cx, y + cy), cxk(k) == 0 || raw);
    }
    const bool lid = gy == 0;
    const bool special = any != 0 || x0 == 0 || x0 + V >= geo.nx || lid || gy == geo.NY - 1;
    if (special && !raw) {
#pragma unroll
        for (int k = 1; k < Q; ++k) {
            const T own = vload<R, V, NT>(src + opp(k) * geo.plane + me, true);
            const int sgy = gy + cyk(k);
            const bool out_y = sgy < 0 || sgy >= geo.NY;
#pragma unroll
            for (int c = 0; c < V; ++c) {
                const int sx = x0 + c - cxk(k);
                if (out_y || sx < 0 || sx >= geo.nx || ((lw[c] >> (k - 1)) & 1)) in[k][c] = own[c];
            }
        }
        if (lid) {
            const T rw = vload<R, V, NT>(src + geo.at(x0, y - 1), true);   // the densities the lid cells parked (wall_rho_at)
#pragma unroll
            for (int c = 0; c < V; ++c) {
                const R t = lid_term<R>(rw[c], w.uLB);
                in[8][c] = in[8][c] + t;
                in[7][c] = in[7][c] - t;
            }
        }
    }
    collide_vec<R, COLL, V, false>(in, w, outv, hq, hr);
    // MOVE: a fluid lane with links adds the delta of link k to its post-collision population of direction opp(k), one add in the lattice
    // type, in the raw first step too.  Only lanes whose link word has a link bit read the table.
    if (any & 255) {
        cell_row += (long long)blockIdx.y * geo.nx * geo.ny + (long long)y * geo.nx + x0;
#pragma unroll
        for (int c = 0; c < V; ++c)
            if ((lw[c] & 255) && !(lw[c] & LINK_SOLID)) {
                const int row = cell_row[c];
                if (row < 0) continue;
                const R* const d = delta + (long long)row * 8;
#pragma unroll
                for (int k = 1; k < Q; ++k)
                    if ((lw[c] >> (k - 1)) & 1) outv[opp(k)][c] = outv[opp(k)][c] + d[k - 1];
            }
    }
    if (any & LINK_SOLID) {
#pragma unroll
        for (int c = 0; c < V; ++c)
            if (lw[c] & LINK_SOLID) {
#pragma unroll
                for (int k = 0; k < Q; ++k) outv[k][c] = weight<R>(k);
            }
    }
#pragma unroll
    for (int k = 0; k < Q; ++k) vstore<R, V, NT>(dst + k * geo.plane + me, outv[k]);
    // park the lid cells' densities for the next step's lid term (update_cell_a; the same sum, the same bits).  A solid lane parks a sum
    // too, where the generic route parks nothing: only that solid cell would read it, and its gather returns the constants before it
    // does -- the ghost rows are not part of the equality of the two routes, the lattice's own cells and every export are.
    if (lid) {
        T rho;
#pragma unroll
        for (int c = 0; c < V; ++c)
            rho[c] = ((((((((in[0][c] + in[1][c]) + in[2][c]) + in[3][c]) + in[4][c]) + in[5][c]) + in[6][c]) + in[7][c]) + in[8][c]);
        vstore<R, V, NT>(dst + geo.at(x0, y - 1), rho);
    }
}

// one thread per cell (kernel = GENERIC, and lattices whose nx is no multiple of the vector width): k_step_generic with MOVE
template <typename R, int COLL>
__global__ __launch_bounds__(BLK) void k_step_generic_move(const R* __restrict__ src, R* __restrict__ dst, Geo geo, Relax<R> w, Batch<R> bt, int raw,
                                                           int row0, int row_stride, const int32_t* __restrict__ cell_row, const R* __restrict__ delta) {
    const int x = blockIdx.x * BLK + threadIdx.x;
    const int y = row0 + blockIdx.y * row_stride;
    if (x >= geo.nx) return;
    LBM_BATCH_SELECT(blockIdx.z)
    update_cell_a<R, COLL, SEM_SOLID, false, Geo, Geo, true>(src, geo, dst, geo, geo, w, raw, x, y, nullptr,
                                                             cell_row + (long long)blockIdx.z * geo.nx * geo.ny, delta);
}

#define LBM_MOVE_ONE(R, COLL)                                                                                                       \
    LBM_MX template __global__ void k_step_solid_move<R, COLL, false>(const R* __restrict__, R* __restrict__, Geo, Relax<R>, Batch<R>, int, int, int, int, \
                                                                     int, const int32_t* __restrict__, const R* __restrict__);    \
    LBM_MX template __global__ void k_step_solid_move<R, COLL, true>(const R* __restrict__, R* __restrict__, Geo, Relax<R>, Batch<R>, int, int, int, int, \
                                                                    int, const int32_t* __restrict__, const R* __restrict__);     \
    LBM_MX template __global__ void k_step_generic_move<R, COLL>(const R* __restrict__, R* __restrict__, Geo, Relax<R>, Batch<R>, int, int, int,       \
                                                                const int32_t* __restrict__, const R* __restrict__);
#define LBM_INST_MOVE(R) \
    LBM_MOVE_ONE(R, C_SRT) LBM_MOVE_ONE(R, C_TRT) LBM_MOVE_ONE(R, C_MRT) LBM_MOVE_ONE(R, C_MRT_FAST) LBM_MOVE_ONE(R, C_SRT_FAST) LBM_MOVE_ONE(R, C_TRT_FAST)
#ifdef LBM_MOVE_INST
#define LBM_MX
LBM_MOVE_INST
#else
#define LBM_MX extern
LBM_INST_MOVE(float) LBM_INST_MOVE(double)
#endif
