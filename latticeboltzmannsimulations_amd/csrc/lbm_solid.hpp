// lbm_solid.hpp -- solid obstacles in the bounce-back cavity (LBM_SEM_BOUNCE_BACK_SOLID; contract in include/lbm.h):
// the one-step vector kernel of a lattice with a solid mask.  The rule itself is gather_a<.., SEM_SOLID> of lbm_device.hpp;
// k_step_generic<.., SEM_SOLID> runs it cell by cell and is what this kernel must equal bit for bit.  Instantiated in
// lbm_solid_f32.hip / lbm_solid_f64.hip (LBM_INST_SOLID below); lbm_solid.hip holds the host side, the kernel that gives solid cells
// their constants and the force reduction.
#pragma once
#include "lbm_kernels.hpp"

// One step of a lattice with solid cells, 16 B per access: a thread owns V consecutive cells of a row (as k_step_vec; blocks dealt to
// the XCDs in bands of rows; lattices of a batch on grid axis y).  It reads its V link words first.  Where they are all zero and the
// cells touch neither a wall nor the lid the step is the plain pull.  Otherwise every slot whose source lies outside the lattice or is
// a solid cell takes the cell's own post-collision population of the opposite direction (one more aligned 16-byte load per direction),
// the lid row adds Ladd's term from the parked density and parks the new one, and solid lanes keep their constants w_k.  Arithmetic
// per cell: collide_vec, the operations of update_cell.
template <typename R, int COLL, bool NT>
__global__ __launch_bounds__(BLK) void k_step_solid(const R* __restrict__ src, R* __restrict__ dst, Geo geo, Relax<R> w, Batch<R> bt, int raw,
                                                    int row0, int row_stride, int nxb, int nblocks) {
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

#define LBM_SOLID_ONE(R, COLL)                                                                                                  \
    LBM_SX template __global__ void k_step_solid<R, COLL, false>(const R* __restrict__, R* __restrict__, Geo, Relax<R>, Batch<R>, int, int, int, int, int); \
    LBM_SX template __global__ void k_step_solid<R, COLL, true>(const R* __restrict__, R* __restrict__, Geo, Relax<R>, Batch<R>, int, int, int, int, int);
#define LBM_INST_SOLID(R) \
    LBM_SOLID_ONE(R, C_SRT) LBM_SOLID_ONE(R, C_TRT) LBM_SOLID_ONE(R, C_MRT) LBM_SOLID_ONE(R, C_MRT_FAST) LBM_SOLID_ONE(R, C_SRT_FAST) LBM_SOLID_ONE(R, C_TRT_FAST)
#ifdef LBM_SOLID_INST
#define LBM_SX
LBM_SOLID_INST
#else
#define LBM_SX extern
LBM_INST_SOLID(float) LBM_INST_SOLID(double)
#endif
