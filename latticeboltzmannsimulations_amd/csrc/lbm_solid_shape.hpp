// lbm_solid_shape.hpp -- the step kernels of a lattice whose solid bodies carry a wall distance per link (lbm_set_solid_shape; contract in
// include/lbm.h): k_step_solid and k_step_generic<.., SEM_SOLID> with the interpolated bounce-back, shape_rule of
// lbm_device.hpp, on the read side of every link.  Launched only while a shape is set, with or without a body motion (whose term is part
// of the table: stores are the pure post-collision values); a context without a shape launches the kernels it always did.  Instantiated
// in lbm_solid_shape_f32.hip / lbm_solid_shape_f64.hip, units of their own, so that the units of k_step_solid, k_step_solid_move,
// k_step_generic and the tile kernel keep their text.
#pragma once
#include "lbm_solid.hpp"

// k_step_solid (lbm_solid.hpp) line for line, but for the block marked SHAPE in the special branch: the cell's eight stored slots are
// loaded first, a lane's link k then takes shape_rule(own = stored opp(k), other = the regular pull of slot opp(k) (near) or stored k
// (far), a, d) from the cell's row of the table (ShapeTable, lbm_device.hpp; the table of lattice blockIdx.y of a batch).  The pulls of a
// near link's slot opp(k) are never overwritten: its source is a fluid cell inside the lattice.  A kernel of its own, as
// k_step_solid_move, for the same reason; the tests hold it to the CPU reference and to the generic route bit for bit.
template <typename R, int COLL, bool NT>
__global__ __launch_bounds__(BLK) void k_step_solid_shape(const R* __restrict__ src, R* __restrict__ dst, Geo geo, Relax<R> w, Batch<R> bt, int raw,
                                                          int row0, int row_stride, int nxb, int nblocks, ShapeTable<R> sh) {
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
        T st[Q];   // the cell's own stored slots
#pragma unroll
        for (int k = 1; k < Q; ++k) st[k] = vload<R, V, NT>(src + k * geo.plane + me, true);
        // SHAPE: the rows of the lanes that have links (fluid lanes only)
        int row[V];
#pragma unroll
        for (int c = 0; c < V; ++c) row[c] = -1;
        if (any & 255) {
            const int32_t* const cr = sh.cell_row + (long long)blockIdx.y * geo.nx * geo.ny + (long long)y * geo.nx + x0;
#pragma unroll
            for (int c = 0; c < V; ++c)
                if ((lw[c] & 255) && !(lw[c] & LINK_SOLID)) row[c] = cr[c];
        }
#pragma unroll
        for (int k = 1; k < Q; ++k) {
            const int sgy = gy + cyk(k);
            const bool out_y = sgy < 0 || sgy >= geo.NY;
#pragma unroll
            for (int c = 0; c < V; ++c) {
                const int sx = x0 + c - cxk(k);
                if (out_y || sx < 0 || sx >= geo.nx) {
                    in[k][c] = st[opp(k)][c];
                } else if ((lw[c] >> (k - 1)) & 1) {
                    if (row[c] >= 0) {
                        const R* const ad = sh.ad + (long long)row[c] * 16;
                        const R other = ((sh.near[row[c]] >> (k - 1)) & 1) ? in[opp(k)][c] : st[k][c];
                        in[k][c] = shape_rule<R>(st[opp(k)][c], other, ad[k - 1], ad[8 + k - 1]);
                    } else {
                        in[k][c] = st[opp(k)][c];
                    }
                }
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
    // park the lid cells' densities for the next step's lid term (as k_step_solid)
    if (lid) {
        T rho;
#pragma unroll
        for (int c = 0; c < V; ++c)
            rho[c] = ((((((((in[0][c] + in[1][c]) + in[2][c]) + in[3][c]) + in[4][c]) + in[5][c]) + in[6][c]) + in[7][c]) + in[8][c]);
        vstore<R, V, NT>(dst + geo.at(x0, y - 1), rho);
    }
}

// one thread per cell (kernel = GENERIC, and lattices whose nx is no multiple of the vector width): k_step_generic with SHAPE
template <typename R, int COLL>
__global__ __launch_bounds__(BLK) void k_step_generic_shape(const R* __restrict__ src, R* __restrict__ dst, Geo geo, Relax<R> w, Batch<R> bt, int raw,
                                                            int row0, int row_stride, ShapeTable<R> sh) {
    const int x = blockIdx.x * BLK + threadIdx.x;
    const int y = row0 + blockIdx.y * row_stride;
    if (x >= geo.nx) return;
    LBM_BATCH_SELECT(blockIdx.z)
    sh.cell_row += (long long)blockIdx.z * geo.nx * geo.ny;
    update_cell_a<R, COLL, SEM_SOLID, false, Geo, Geo, false, true>(src, geo, dst, geo, geo, w, raw, x, y, nullptr, nullptr, nullptr, sh);
}

#define LBM_SHAPE_ONE(R, COLL)                                                                                                                              \
    LBM_HX template __global__ void k_step_solid_shape<R, COLL, false>(const R* __restrict__, R* __restrict__, Geo, Relax<R>, Batch<R>, int, int, int, int, \
                                                                      int, ShapeTable<R>);                                                                \
    LBM_HX template __global__ void k_step_solid_shape<R, COLL, true>(const R* __restrict__, R* __restrict__, Geo, Relax<R>, Batch<R>, int, int, int, int,  \
                                                                     int, ShapeTable<R>);                                                                 \
    LBM_HX template __global__ void k_step_generic_shape<R, COLL>(const R* __restrict__, R* __restrict__, Geo, Relax<R>, Batch<R>, int, int, int, ShapeTable<R>);
#define LBM_INST_SHAPE(R) \
    LBM_SHAPE_ONE(R, C_SRT) LBM_SHAPE_ONE(R, C_TRT) LBM_SHAPE_ONE(R, C_MRT) LBM_SHAPE_ONE(R, C_MRT_FAST) LBM_SHAPE_ONE(R, C_SRT_FAST) LBM_SHAPE_ONE(R, C_TRT_FAST)
#ifdef LBM_SHAPE_INST
#define LBM_HX
LBM_SHAPE_INST
#else
#define LBM_HX extern
LBM_INST_SHAPE(float) LBM_INST_SHAPE(double)
#endif
