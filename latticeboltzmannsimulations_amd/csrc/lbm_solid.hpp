// lbm_solid.hpp -- solid obstacles in the bounce-back cavity (LBM_SEM_BOUNCE_BACK_SOLID; contract in include/lbm.h):
// the one-step kernels of a lattice with a solid mask, one template for every mode of the wall rule -- a base (WALL_REST, WALL_MOVE,
// WALL_SHAPE) | the bits of buoyancy, the sub-grid closure and a relaxation field (WallArg, lbm_device.hpp).  The rule itself is
// gather_a<.., SEM_SOLID> and update_cell_a of lbm_device.hpp, which k_step_generic<.., SEM_SOLID> (at rest) and k_step_generic_wall (every
// other mode, and a driving force) run cell by cell; the vector kernel must equal them bit for bit.  Instantiated per mode and real type
// by the one macro LBM_INST_SOLID below, a unit per mode and type that compile in parallel: lbm_solid{,_move,_shape}_f32/f64.hip the bases,
// lbm_solid_buoy_* WALL_BUOY on the modes at rest and with a motion, lbm_solid_sgs{,_move,_shape}_* WALL_SGS, lbm_solid_relax{,_move,_shape}_*
// WALL_RELAX, lbm_solid_relax_sgs{,_move,_shape}_* both, lbm_solid_rheo{,_move,_shape}_* WALL_RHEO; lbm_solid.hip holds the host side, the kernel that gives solid cells their
// constants and the force reduction.
// The mode blocks sit under `if constexpr` of the kernel template itself, so every mode's kernel is the text it would have alone (a
// shared __forceinline__ body with a bool switch was tried first and changed the register allocation of the kernel at rest: DESIGN.md 2.10).
#pragma once
#include "lbm_kernels.hpp"

// One step of a lattice with solid cells, 16 B per access: a thread owns V consecutive cells of a row (as k_step_vec; blocks dealt to
// the XCDs in bands of rows; lattices of a batch on grid axis y).  It reads its V link words first.  Where they are all zero and the
// cells touch neither a wall nor the lid the step is the plain pull.  Otherwise every slot whose source lies outside the lattice or is
// a solid cell takes the cell's own post-collision population of the opposite direction (one more aligned 16-byte load per direction),
// the lid row adds Ladd's term from the parked density and parks the new one, and solid lanes keep their constants w_k, hold lanes (bit
// LINK_HOLD of the link word) the values they hold.  Arithmetic per cell: collide_vec, the operations of update_cell.
//   WALL_SHAPE  the cell's eight stored slots are loaded first; a lane's link k then takes shape_rule(own = stored opp(k), other = the
//               regular pull of slot opp(k) (near) or stored k (far), a, d) from the cell's row of the table.  The pull of a near link's
//               slot opp(k) is never overwritten: its source is a fluid cell inside the lattice.  (shape_link of lbm_device.hpp loads
//               `other`; here both candidates are in registers already, so the choice is spelled in place.)
//   WALL_MOVE   between the collision and the pinning of the solid lanes a fluid lane with links adds the delta of link k to its
//               post-collision population of direction opp(k), one add in the lattice type, in the raw first step too.  Only lanes
//               whose link word has a link bit read the table.
//   dr          the driving force (lbm_set_driving_force; Drive, lbm_device.hpp): while bit SOLID_DRIVE of the argument raw_drive is set,
//               every lane adds F_k to its post-collision population of direction k, one add in the lattice type, before the delta of
//               WALL_MOVE and before the solid and the hold lanes are pinned; a uniform run-time test, no template parameter (DESIGN.md
//               2.10).  The vector kernel never reads dr.on, which the one-cell route tests.
//   WALL_BUOY   (lbm_set_buoyancy; Buoy, lbm_device.hpp) one more aligned 16-byte load, the cells' values of the buoyancy plane, next to
//               the link words; in the place of the driving force every lane adds d_k = F_k + B_k (Cp - c_ref) to its post-collision
//               population of direction k: t per lane, d_k per lane and slot, one add, all in the lattice type.
//   WALL_SGS    (lbm_set_subgrid, subgrid_tau of lbm_device.hpp) no load and no store more: collide_vec forms every lane's tau from the
//               lane's gathered populations and its moments -- the MRT operators then form the velocity too -- and takes 1 / tau into the
//               collision in the place of the lattice's rate.  Solid and hold lanes compute a tau that nobody uses and are pinned as ever.
//   WALL_RELAX  (lbm_set_relaxation_field) one more aligned 16-byte load per plane next to the link words -- the cells' viscous rates, and
//               TRT's odd rates where that plane is set (a wave-uniform test of the pointer; the lattice's w_m in every lane otherwise):
//               collide_vec takes each lane's own rates into the collision, with WALL_SGS as the closure's omega.  Solid and hold lanes
//               load rates that nobody uses and are pinned as ever; the force and the wall deltas are added after the collision, unchanged.
//   WALL_RHEO   (lbm_set_rheology, rheology_rates of lbm_device.hpp) no plane and no store more: collide_vec forms every lane's shear from
//               the lane's gathered populations and its moments -- the MRT operators then form the velocity too --, gathers the rates'
//               values and slopes from the context's table, one small load per rate and lane, and takes the interpolated rates into the
//               collision.  Solid and hold lanes look up rates that nobody uses (the index is safe for any value) and are pinned as ever.
constexpr int SOLID_DRIVE = 2;
template <typename R, int COLL, bool NT, int WALL>
__global__ __launch_bounds__(BLK) void k_step_solid(const R* __restrict__ src, R* __restrict__ dst, Geo geo, Relax<R> w, Batch<R> bt, int raw_drive,
                                                    int row0, int row_stride, int nxb, int nblocks, WallArg<R, WALL> wa, Drive<R> dr) {
    constexpr int V = 16 / (int)sizeof(R);
    // bit 0: the lattice is raw; bit 1 (SOLID_DRIVE): a driving force is set.  The flag rides in the word every thread reads first, so
    // a context without a force waits for no scalar load of its own behind the collision (160^2: DESIGN.md 2.10)
    const int raw = raw_drive & 1;
    typedef typename VecT<R, V>::type T;
    LBM_BATCH_SELECT(blockIdx.y)
    const int b = xcd_band(blockIdx.x, nblocks);
    const int y = row0 + (b / nxb) * row_stride, gy = geo.y0 + y;
    const int x0 = ((b % nxb) * BLK + threadIdx.x) * V;
    if (x0 >= geo.nx) return;
    const long long me = geo.at(x0, y);
    const T lk = vload<R, V, NT>(src + K_LINK * geo.plane + me, true);
    T cpv;   // (buoyancy: the cells' values of the buoyancy plane)
    if constexpr (wall_buoyant(WALL)) cpv = vload<R, V, NT>(wa.by.cp + buoy_at(geo, x0, y), true);
    T rwv{}, rmv{};   // (a relaxation field: the cells' own rates)
    if constexpr (wall_relax(WALL)) {
        const long long at = (long long)blockIdx.y * buoy_elems(geo) + buoy_at(geo, x0, y);
        rwv = vload<R, V, false>(wa.rw + at, true);
        if (wa.rwm) {
            rmv = vload<R, V, false>(wa.rwm + at, true);
        } else {
#pragma unroll
            for (int c = 0; c < V; ++c) rmv[c] = w.w_m;
        }
    }
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
        if constexpr (wall_base(WALL) == WALL_SHAPE) {
            T st[Q];   // the cell's own stored slots
#pragma unroll
            for (int k = 1; k < Q; ++k) st[k] = vload<R, V, NT>(src + k * geo.plane + me, true);
            // the rows of the lanes that have links (fluid lanes only)
            int row[V];
#pragma unroll
            for (int c = 0; c < V; ++c) row[c] = -1;
            if (any & 255) {
                const int32_t* const cr = wa.sh.cell_row + batch_cells(blockIdx.y, geo) + (long long)y * geo.nx + x0;
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
                            const R* const ad = wa.sh.ad + (long long)row[c] * 16;
                            const R other = ((wa.sh.near[row[c]] >> (k - 1)) & 1) ? in[opp(k)][c] : st[k][c];
                            in[k][c] = shape_rule<R>(st[opp(k)][c], other, ad[k - 1], ad[8 + k - 1]);
                        } else {
                            in[k][c] = st[opp(k)][c];
                        }
                    }
                }
            }
        } else {   // (at rest, and a motion: its term is on the store side)
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
    R sgs = R(0);   // (the closure: its constant)
    if constexpr (wall_subgrid(WALL)) sgs = wa.sgs;
    if constexpr (wall_rheo(WALL)) collide_vec<R, COLL, V, false, false, false, true, Rheo<R>>(in, w, outv, hq, hr, false, false, 0, R(0), T{}, T{}, wa.rh);
    else collide_vec<R, COLL, V, false, wall_subgrid(WALL), wall_relax(WALL)>(in, w, outv, hq, hr, false, false, 0, sgs, rwv, rmv);
    // the driving force (lbm_set_driving_force), a uniform run-time test: every lane adds F_k, one add in the lattice type; the solid and
    // the hold lanes are pinned below, so the sums of fluid lanes alone are stored
    if constexpr (wall_buoyant(WALL)) {
        // buoyancy (lbm_set_buoyancy; Buoy, lbm_device.hpp): t = Cp - c_ref per lane, d_k = F_k + B_k t per lane and slot, one add of d_k;
        // F_k are zeros without a driving force, so bit SOLID_DRIVE is not read
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const R t = cpv[c] - wa.by.c_ref;
#pragma unroll
            for (int k = 1; k < Q; ++k) {
                const R d = dr.f[k - 1] + wa.by.b[k - 1] * t;
                outv[k][c] = outv[k][c] + d;
            }
        }
    } else if (raw_drive & SOLID_DRIVE) {
#pragma unroll
        for (int k = 1; k < Q; ++k) {
#pragma unroll
            for (int c = 0; c < V; ++c) outv[k][c] = outv[k][c] + dr.f[k - 1];
        }
    }
    if constexpr (wall_base(WALL) == WALL_MOVE) {
        if (any & 255) {
            const int32_t* cell_row = wa.cell_row;
            const R* const delta = wa.delta;
            cell_row += batch_cells(blockIdx.y, geo) + (long long)y * geo.nx + x0;
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
    }
    if (any & LINK_SOLID) {
#pragma unroll
        for (int c = 0; c < V; ++c)
            if (lw[c] & LINK_SOLID) {
#pragma unroll
                for (int k = 0; k < Q; ++k) outv[k][c] = weight<R>(k);
            }
    }
    // a hold lane (lbm_set_open_cells) keeps the nine values the cell holds: its own stored slots, so the 16-byte stores stay whole
    if (any & LINK_HOLD) {
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            const T own = vload<R, V, NT>(src + k * geo.plane + me, true);
#pragma unroll
            for (int c = 0; c < V; ++c)
                if (lw[c] & LINK_HOLD) outv[k][c] = own[c];
        }
    }
#pragma unroll
    for (int k = 0; k < Q; ++k) vstore<R, V, NT>(dst + k * geo.plane + me, outv[k]);
    // park the lid cells' densities for the next step's lid term (update_cell_a; the same sum, the same bits).  A solid lane parks a sum
    // too, where the generic route parks nothing: only that solid cell would read it, and its gather returns the constants before it
    // does -- the ghost rows are not part of the equality of the two routes, the lattice's own cells and every export are.  A hold lane
    // likewise: its gather returns the held values and never reads what it parked.
    if (lid) {
        T rho;
#pragma unroll
        for (int c = 0; c < V; ++c)
            rho[c] = ((((((((in[0][c] + in[1][c]) + in[2][c]) + in[3][c]) + in[4][c]) + in[5][c]) + in[6][c]) + in[7][c]) + in[8][c]);
        vstore<R, V, NT>(dst + geo.at(x0, y - 1), rho);
    }
}

// One thread per cell (kernel = GENERIC, and lattices whose nx is no multiple of the vector width) while a motion, a shape or a driving
// force is set: k_step_generic<.., SEM_SOLID> with the mode and the force of update_cell_a.  At rest and without a force k_step_generic
// itself is what launches.  update_cell_a runs in the base mode, on the mode's tables narrowed once, with one switch and one argument per
// bit: the closure's constant, the cell's own rates, and with buoyancy a Drive of the cell's own, d_k = F_k + B_k (Cp - c_ref) with on = 1
// -- which is why the rule is spelled f* + (F + B t).
template <typename R, int COLL, int WALL>
__global__ __launch_bounds__(BLK) void k_step_generic_wall(const R* __restrict__ src, R* __restrict__ dst, Geo geo, Relax<R> w, Batch<R> bt, int raw,
                                                           int row0, int row_stride, WallArg<R, WALL> wa, Drive<R> dr) {
    const int x = blockIdx.x * BLK + threadIdx.x;
    const int y = row0 + blockIdx.y * row_stride;
    if (x >= geo.nx) return;
    LBM_BATCH_SELECT(blockIdx.z)
    constexpr int BASE = wall_base(WALL);
    if constexpr (WALL == BASE) {   // (no bits: the mode's own tables, offset in place)
        wall_batch(wa, blockIdx.z, geo);
        update_cell_a<R, COLL, SEM_SOLID, false, Geo, Geo, WALL>(src, geo, dst, geo, geo, w, raw, x, y, nullptr, wa, dr);
    } else {
        // update_cell_a in the base mode: the mode's tables, narrowed once, and what each bit of the mode adds.  Member by member, and in
        // this function's own text: a copy of the part as a whole, or a helper that returns the narrowed tables, changes the register
        // allocation of some of these kernels, and so does a narrowed copy in the modes without bits
        WallArg<R, BASE> wb{};
        if constexpr (BASE == WALL_MOVE) wb.cell_row = wa.cell_row, wb.delta = wa.delta;
        if constexpr (BASE == WALL_SHAPE) wb.sh = wa.sh;
        Drive<R> own;   // (buoyancy, a lone lattice: the cell's own force d_k = F_k + B_k (Cp - c_ref) as the driving force)
        if constexpr (wall_buoyant(WALL)) {
            const R t = wa.by.cp[buoy_at(geo, x, y)] - wa.by.c_ref;
#pragma unroll
            for (int k = 0; k < 8; ++k) own.f[k] = dr.f[k] + wa.by.b[k] * t;
            own.on = 1;
        } else {
            wall_batch(wb, blockIdx.z, geo);
        }
        R sgs = R(0), rw = R(0), rwm = R(0);
        if constexpr (wall_relax(WALL)) {   // (a relaxation field: the cell's own rates)
            const long long at = (long long)blockIdx.z * buoy_elems(geo) + buoy_at(geo, x, y);
            rw = wa.rw[at];
            rwm = wa.rwm ? wa.rwm[at] : w.w_m;
        }
        if constexpr (wall_subgrid(WALL)) sgs = wa.sgs;   // (the sub-grid closure: its constant)
        if constexpr (wall_rheo(WALL))   // (a rheology table: the context's)
            update_cell_a<R, COLL, SEM_SOLID, false, Geo, Geo, BASE, false, false, true, Rheo<R>>(src, geo, dst, geo, geo, w, raw, x, y, nullptr, wb, dr, sgs, rw, rwm,
                                                                                         wa.rh);
        else
            update_cell_a<R, COLL, SEM_SOLID, false, Geo, Geo, BASE, wall_subgrid(WALL), wall_relax(WALL)>(src, geo, dst, geo, geo, w, raw, x, y, nullptr, wb,
                                                                                                           wall_buoyant(WALL) ? own : dr, sgs, rw, rwm);
    }
}

// LBM_INST_SOLID(R, WALL): the six operator variants of one real type and mode -- the vector kernel with and without non-temporal
// accesses, and k_step_generic_wall (LBM_SX: `extern`, or nothing in the unit that compiles them)
#define LBM_SOLID_ONE(R, COLL, WALL)                                                                                                                          \
    LBM_SX template __global__ void k_step_solid<R, COLL, false, WALL>(const R* __restrict__, R* __restrict__, Geo, Relax<R>, Batch<R>, int, int, int, int, int, \
                                                                       WallArg<R, WALL>, Drive<R>);                                                           \
    LBM_SX template __global__ void k_step_solid<R, COLL, true, WALL>(const R* __restrict__, R* __restrict__, Geo, Relax<R>, Batch<R>, int, int, int, int, int,  \
                                                                      WallArg<R, WALL>, Drive<R>);                                                            \
    LBM_SX template __global__ void k_step_generic_wall<R, COLL, WALL>(const R* __restrict__, R* __restrict__, Geo, Relax<R>, Batch<R>, int, int, int,             \
                                                                      WallArg<R, WALL>, Drive<R>);
#define LBM_INST_SOLID(R, WALL)                                                                                                  \
    LBM_SOLID_ONE(R, C_SRT, WALL) LBM_SOLID_ONE(R, C_TRT, WALL) LBM_SOLID_ONE(R, C_MRT, WALL) LBM_SOLID_ONE(R, C_MRT_FAST, WALL) \
    LBM_SOLID_ONE(R, C_SRT_FAST, WALL) LBM_SOLID_ONE(R, C_TRT_FAST, WALL)
#ifdef LBM_SOLID_INST
#define LBM_SX
LBM_SOLID_INST
#else
#define LBM_SX extern
LBM_INST_SOLID(float, WALL_REST) LBM_INST_SOLID(double, WALL_REST)
LBM_INST_SOLID(float, WALL_MOVE) LBM_INST_SOLID(double, WALL_MOVE)
LBM_INST_SOLID(float, WALL_SHAPE) LBM_INST_SOLID(double, WALL_SHAPE)
LBM_INST_SOLID(float, WALL_REST | WALL_BUOY) LBM_INST_SOLID(double, WALL_REST | WALL_BUOY)
LBM_INST_SOLID(float, WALL_MOVE | WALL_BUOY) LBM_INST_SOLID(double, WALL_MOVE | WALL_BUOY)
LBM_INST_SOLID(float, WALL_REST | WALL_SGS) LBM_INST_SOLID(double, WALL_REST | WALL_SGS)
LBM_INST_SOLID(float, WALL_MOVE | WALL_SGS) LBM_INST_SOLID(double, WALL_MOVE | WALL_SGS)
LBM_INST_SOLID(float, WALL_SHAPE | WALL_SGS) LBM_INST_SOLID(double, WALL_SHAPE | WALL_SGS)
LBM_INST_SOLID(float, WALL_REST | WALL_RELAX) LBM_INST_SOLID(double, WALL_REST | WALL_RELAX)
LBM_INST_SOLID(float, WALL_MOVE | WALL_RELAX) LBM_INST_SOLID(double, WALL_MOVE | WALL_RELAX)
LBM_INST_SOLID(float, WALL_SHAPE | WALL_RELAX) LBM_INST_SOLID(double, WALL_SHAPE | WALL_RELAX)
LBM_INST_SOLID(float, WALL_REST | WALL_SGS | WALL_RELAX) LBM_INST_SOLID(double, WALL_REST | WALL_SGS | WALL_RELAX)
LBM_INST_SOLID(float, WALL_MOVE | WALL_SGS | WALL_RELAX) LBM_INST_SOLID(double, WALL_MOVE | WALL_SGS | WALL_RELAX)
LBM_INST_SOLID(float, WALL_SHAPE | WALL_SGS | WALL_RELAX) LBM_INST_SOLID(double, WALL_SHAPE | WALL_SGS | WALL_RELAX)
LBM_INST_SOLID(float, WALL_REST | WALL_RHEO) LBM_INST_SOLID(double, WALL_REST | WALL_RHEO)
LBM_INST_SOLID(float, WALL_MOVE | WALL_RHEO) LBM_INST_SOLID(double, WALL_MOVE | WALL_RHEO)
LBM_INST_SOLID(float, WALL_SHAPE | WALL_RHEO) LBM_INST_SOLID(double, WALL_SHAPE | WALL_RHEO)
#endif
