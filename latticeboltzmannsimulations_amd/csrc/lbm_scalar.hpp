// lbm_scalar.hpp -- a passive scalar (temperature, dye) carried by the flow of an obstacle lattice (lbm_scalar_*; contract in
// include/lbm.h): a second set of nine populations g_k on the flow's own D2Q9 stencil, advection-diffusion by a TRT
// collision about geq_k = w_k C (1 + 3 c_k.u), half-way walls that are adiabatic (bounce-back) or hold a value (anti-bounce-back).  The
// scalar lattices have the flow's layout (Geo) and no link plane: every kernel here reads plane K_LINK of the flow lattice.
//   host part    the relaxation rates, the wall-value table and the constants of the hold cells, in plain C++ (nothing from HIP:
//                tests/test_scalar_cpu.py drives it from a program of its own); arrays in the host layout of the mask, [nx][ny], y fastest
//   device part  (under __HIPCC__) scalar_gather and scalar_collide, the rule of one cell (scalar_cell), the one-cell kernel
//                k_scalar_generic and the vector kernel k_scalar_step, which must equal it bit for bit; the export, the totals, the flux
// One lattice, one step per launch.  No existing kernel knows of the scalar: a context without one launches what it always did.  With
// buoyancy (lbm_set_buoyancy) the step also stores the C it sums into the buoyancy plane the next flow step reads: k_scalar_generic_cp,
// k_scalar_step_cp; k_scalar_plane fills the plane from a lattice as it is.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "lbm_devmem.hpp"
#include "lbm_wall_motion.hpp"   // (BODY_CX, BODY_CY; LBM_WM_ATTR, LBM_WM_NO_CONTRACT)

namespace lbmhost {

// The two rates of the scalar's TRT collision from the diffusivity D and the product magic = (1/w+ - 1/2)(1/w- - 1/2), in double, every
// operation rounded in the order written:  tm = 3 D + 1/2;  w- = 1 / tm;  tp = magic / (tm - 1/2) + 1/2;  w+ = 1 / tp.  The caller
// rounds each once to the lattice type.  BGK is magic = (3 D)^2.
LBM_WM_ATTR inline void scalar_rates(double D, double magic, double* w_plus, double* w_minus) {
    LBM_WM_NO_CONTRACT
    const double tm = 3.0 * D + 0.5;
    const double tp = magic / (tm - 0.5) + 0.5;
    *w_minus = 1.0 / tm;
    *w_plus = 1.0 / tp;
}

// the lattice weights as the lattice type rounds them (weight<R> of lbm_device.hpp, in double)
inline double scalar_weight(int k) { return k == 0 ? 4.0 / 9.0 : (k < 5 ? 1.0 / 9.0 : 1.0 / 36.0); }

// The wall values of one lattice: one row per fluid cell (neither solid nor held) that has a link to a Dirichlet solid cell.
//   cell_row[ny][nx], x fastest (as the lattice's rows): -1, or the cell's row
//   val[rows][8]     slot k - 1: 2 w_k Cw(S) of the cell's link k, S = (x - cx_k, y + cy_k) its source, in double (the caller rounds each
//                    once to the lattice type); 0 where link k is none or adiabatic
//   bits[rows]       bit k - 1: link k is a Dirichlet link (a value of 0 is a value)
// mask, hold (null: none; the flow's hold cells, image cells included), dirichlet (null: none) are 0 / 1, wall_value is read on Dirichlet
// cells only.
struct ScalarWalls {
    std::vector<int32_t> cell_row;
    std::vector<double> val;
    std::vector<uint8_t> bits;
};
LBM_WM_ATTR inline ScalarWalls scalar_wall_table(const uint8_t* mask, const uint8_t* hold, const uint8_t* dirichlet, const double* wall_value, int nx,
                                                 int ny) {
    LBM_WM_NO_CONTRACT
    ScalarWalls t;
    t.cell_row.assign((size_t)nx * ny, -1);
    if (!dirichlet) return t;
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            const size_t i = (size_t)x * ny + y;
            if (mask[i] || (hold && hold[i])) continue;
            int row = -1;
            for (int k = 1; k < 9; ++k) {
                const int sx = x - BODY_CX[k], sy = y + BODY_CY[k];
                if (sx < 0 || sx >= nx || sy < 0 || sy >= ny) continue;
                const size_t s = (size_t)sx * ny + sy;
                if (!mask[s] || !dirichlet[s]) continue;
                if (row < 0) {
                    row = (int)t.bits.size();
                    t.cell_row[(size_t)y * nx + x] = row;
                    t.bits.push_back(0);
                    t.val.resize(t.val.size() + 8, 0.0);
                }
                t.bits[(size_t)row] |= (uint8_t)(1u << (k - 1));
                t.val[(size_t)row * 8 + (k - 1)] = (2.0 * scalar_weight(k)) * wall_value[s];
            }
        }
    return t;
}

// What a user's hold cell keeps: g_k = (w_k Ch) (1 + 3 (cx_k ux + cy_k uy)), k = 0 .. 8, in double in the order written, (ux, uy) the
// moments of the nine flow populations f the cell holds, summed in the order of the flow's density and momenta.  The caller rounds each
// once to the lattice type.
LBM_WM_ATTR inline void scalar_hold_values(const double* f, double Ch, double (&out)[9]) {
    LBM_WM_NO_CONTRACT
    const double rho = ((((((((f[0] + f[1]) + f[2]) + f[3]) + f[4]) + f[5]) + f[6]) + f[7]) + f[8]);
    const double ux = (((((f[1] - f[3]) + f[5]) - f[6]) - f[7]) + f[8]) / rho;
    const double uy = (((((f[2] - f[4]) + f[5]) + f[6]) - f[7]) - f[8]) / rho;
    for (int k = 0; k < 9; ++k) out[k] = (scalar_weight(k) * Ch) * (1.0 + 3.0 * ((double)BODY_CX[k] * ux + (double)BODY_CY[k] * uy));
}
}  // namespace lbmhost

#ifdef __HIPCC__
#include "lbm_fields.hpp"
#include "lbm_periodic.hpp"
#include "lbm_reduce.hpp"

// What the scalar kernels take by value: the two rates in the lattice type and the wall-value table (ScalarWalls, val rounded to the
// lattice type).
template <typename R>
struct ScalarArg {
    R w_plus, w_minus;
    const int32_t* cell_row;
    const R* val;
    const uint8_t* bits;
};

// The arriving populations of cell (x, y) from a scalar lattice that holds post-collision values, lw the cell's word of the flow's link
// plane.  A solid cell: zeros.  raw (plain populations: the state just set) and hold cells: the nine stored values.  Otherwise slot k
// pulls from (x - cx_k, y + cy_k); a source outside the lattice gives the cell's own stored slot opp(k) (adiabatic: the box and the lid); a
// source that is a solid cell gives own = stored opp(k) (adiabatic) or t - own, t = 2 w_k Cw of the cell's row (Dirichlet).
template <typename R>
__device__ __forceinline__ void scalar_gather(const R* __restrict__ s, const Geo& geo, int lw, int raw, int x, int y, const ScalarArg<R>& a, R (&g)[Q]) {
    if (lw & LINK_SOLID) {
#pragma unroll
        for (int k = 0; k < Q; ++k) g[k] = (R)0;
        return;
    }
    const long long me = geo.at(x, y);
    if (raw || (lw & LINK_HOLD)) {
#pragma unroll
        for (int k = 0; k < Q; ++k) g[k] = s[k * geo.plane + me];
        return;
    }
#pragma unroll
    for (int k = 0; k < Q; ++k) g[k] = s[k * geo.plane + geo.at(x - cxk(k), y + cyk(k))];
    const bool edge = x == 0 || x == geo.nx - 1 || y == 0 || y == geo.ny - 1;
    if (!edge && !(lw & 255)) return;
    const int row = (lw & 255) ? a.cell_row[(long long)y * geo.nx + x] : -1;
    const unsigned db = row >= 0 ? a.bits[row] : 0u;
#pragma unroll
    for (int k = 1; k < Q; ++k) {
        const int sx = x - cxk(k), sy = y + cyk(k);
        const bool out = sx < 0 || sx >= geo.nx || sy < 0 || sy >= geo.ny;
        if (!out && !((lw >> (k - 1)) & 1)) continue;
        const R own = s[opp(k) * geo.plane + me];
        g[k] = (!out && ((db >> (k - 1)) & 1u)) ? a.val[(long long)row * 8 + (k - 1)] - own : own;
    }
}

// The collision, on a scalar real or on a vector of them (lane-wise IEEE, the same bits), every operation in the lattice type in the
// order written:  C = sum g in the order of the flow's density;  out_0 = g_0 - w+ (g_0 - w_0 C);  for the pairs (a, b) = (1, 3), (2, 4),
// (5, 7), (6, 8), with cu = c_a.u spelled as the flow's cu_of:
//     gp = (g_a + g_b) / 2;  gm = (g_a - g_b) / 2;  e = w_a C;  dp = w+ (gp - e);  dm = w- (gm - (3 e) cu);
//     out_a = (g_a - dp) - dm;  out_b = (g_b - dp) + dm
template <typename T, typename R>
__device__ __forceinline__ void scalar_collide(const T (&g)[Q], T ux, T uy, R wp, R wm, T (&out)[Q], T& C) {
    C = ((((((((g[0] + g[1]) + g[2]) + g[3]) + g[4]) + g[5]) + g[6]) + g[7]) + g[8]);
    out[0] = g[0] - (g[0] - C * weight<R>(0)) * wp;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int a = p < 2 ? p + 1 : p + 3, b = opp(a);
        const T cu = cu_of<T>(a, ux, uy);
        const T gp = (g[a] + g[b]) * (R)0.5, gm = (g[a] - g[b]) * (R)0.5;
        const T e = C * weight<R>(a);
        const T dp = (gp - e) * wp, dm = (gm - (e * (R)3) * cu) * wm;
        out[a] = (g[a] - dp) - dm;
        out[b] = (g[b] - dp) + dm;
    }
}

// One scalar step of cell (x, y): the definition.  f: the view of the flow lattice the flow step has just written, whose link plane and
// whose velocity (Fields::macro: what lbm_get_fields exports after the next step, in the lattice type) the scalar takes.  A solid cell and
// a hold cell are never written: both scalar lattices hold their constants (zeros; the held values), and the wrap refreshes an image.
// CP (buoyancy, lbm_set_buoyancy): the C the collision summed goes into the buoyancy plane cp as well (buoy_at, lbm_device.hpp); a
// solid cell and a hold cell keep what the fill wrote there (k_scalar_plane).
template <typename R, bool SHAPE, bool CP = false>
__device__ __forceinline__ void scalar_cell(const R* __restrict__ src, R* __restrict__ dst, const Fields<R, SEM_SOLID, false, SHAPE>& f,
                                            const ScalarArg<R>& a, int raw, int x, int y, R* __restrict__ cp = nullptr) {
    const Geo& geo = f.geo;
    const long long me = geo.at(x, y);
    const int lw = (int)f.src[K_LINK * geo.plane + me];
    if (lw & (LINK_SOLID | LINK_HOLD)) return;
    R g[Q], out[Q], ux, uy, rho, C;
    scalar_gather<R>(src, geo, lw, raw, x, y, a, g);
    f.macro(x, y, ux, uy, rho);
    scalar_collide<R, R>(g, ux, uy, a.w_plus, a.w_minus, out, C);
#pragma unroll
    for (int k = 0; k < Q; ++k) dst[k * geo.plane + me] = out[k];
    if constexpr (CP) cp[buoy_at(geo, x, y)] = C;
}

// One thread per cell: kernel = GENERIC, and lattices whose nx is no multiple of the vector width.
template <typename R, bool SHAPE>
__global__ __launch_bounds__(BLK) void k_scalar_generic(const R* __restrict__ src, R* __restrict__ dst, Fields<R, SEM_SOLID, false, SHAPE> f, ScalarArg<R> a,
                                                        int raw) {
    const int x = blockIdx.x * BLK + threadIdx.x, y = blockIdx.y;
    if (x >= f.geo.nx) return;
    scalar_cell<R, SHAPE>(src, dst, f, a, raw, x, y);
}
// ... and with buoyancy (no shape): the same step, C into the buoyancy plane too
template <typename R>
__global__ __launch_bounds__(BLK) void k_scalar_generic_cp(const R* __restrict__ src, R* __restrict__ dst, Fields<R, SEM_SOLID, false, false> f, ScalarArg<R> a,
                                                           int raw, R* __restrict__ cp) {
    const int x = blockIdx.x * BLK + threadIdx.x, y = blockIdx.y;
    if (x >= f.geo.nx) return;
    scalar_cell<R, false, true>(src, dst, f, a, raw, x, y, cp);
}

// 16 B per access, the shape of k_step_solid: a thread owns V consecutive cells of a row and reads their V link words first.  Where they
// are all zero and the cells touch no edge of the box the step is the plain pull; otherwise one more aligned load per direction for the
// own opposite slots, and the table for the lanes with Dirichlet links.  The velocity of every lane comes through the view, as in
// scalar_cell.  Solid lanes store zeros, hold lanes what they hold, so the 16-byte stores stay whole.
template <typename R, bool NT, bool SHAPE>
__global__ __launch_bounds__(BLK) void k_scalar_step(const R* __restrict__ src, R* __restrict__ dst, Fields<R, SEM_SOLID, false, SHAPE> f, ScalarArg<R> a,
                                                     int raw, int nxb, int nblocks) {
    constexpr int V = 16 / (int)sizeof(R);
    typedef typename VecT<R, V>::type T;
    const Geo& geo = f.geo;
    const int b = xcd_band(blockIdx.x, nblocks);
    const int y = b / nxb;
    const int x0 = ((b % nxb) * BLK + threadIdx.x) * V;
    if (x0 >= geo.nx) return;
    const long long me = geo.at(x0, y);
    const T lk = vload<R, V, false>(f.src + K_LINK * geo.plane + me, true);
    int lw[V], any = 0;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        lw[c] = (int)lk[c];
        any |= lw[c];
    }
    T in[Q], outv[Q];
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        const int cx = raw ? 0 : cxk(k), cy = raw ? 0 : cyk(k);
        in[k] = vload<R, V, NT>(src + k * geo.plane + geo.at(x0 - cx, y + cy), cxk(k) == 0 || raw);
    }
    const bool special = any != 0 || x0 == 0 || x0 + V >= geo.nx || y == 0 || y == geo.ny - 1;
    if (special && !raw) {
        int row[V];
#pragma unroll
        for (int c = 0; c < V; ++c) row[c] = -1;
        if (any & 255) {
            const int32_t* const cr = a.cell_row + (long long)y * geo.nx + x0;
#pragma unroll
            for (int c = 0; c < V; ++c)
                if ((lw[c] & 255) && !(lw[c] & (LINK_SOLID | LINK_HOLD))) row[c] = cr[c];
        }
#pragma unroll
        for (int k = 1; k < Q; ++k) {
            const T own = vload<R, V, NT>(src + opp(k) * geo.plane + me, true);
            const int sy = y + cyk(k);
            const bool out_y = sy < 0 || sy >= geo.ny;
#pragma unroll
            for (int c = 0; c < V; ++c) {
                const int sx = x0 + c - cxk(k);
                if (out_y || sx < 0 || sx >= geo.nx) {
                    in[k][c] = own[c];
                } else if ((lw[c] >> (k - 1)) & 1) {
                    const bool dir = row[c] >= 0 && ((a.bits[row[c]] >> (k - 1)) & 1u);
                    in[k][c] = dir ? a.val[(long long)row[c] * 8 + (k - 1)] - own[c] : own[c];
                }
            }
        }
    }
    T ux, uy, C;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        R u, v, rho;
        f.macro(x0 + c, y, u, v, rho);
        ux[c] = u;
        uy[c] = v;
    }
    scalar_collide<T, R>(in, ux, uy, a.w_plus, a.w_minus, outv, C);
    if (any & LINK_SOLID) {
#pragma unroll
        for (int c = 0; c < V; ++c)
            if (lw[c] & LINK_SOLID) {
#pragma unroll
                for (int k = 0; k < Q; ++k) outv[k][c] = (R)0;
            }
    }
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
}
// ... and with buoyancy (lbm_set_buoyancy; no shape): the same step with one more 16-byte store.  A kernel text of its own: the passive
// kernel above keeps the text it had, so its code is what it was (a body shared through a __forceinline__ function changed its register
// allocation, as lbm_solid.hpp found for the flow's).  tests/test_buoyancy_gpu.py holds the two to the same bits through the reference.
template <typename R, bool NT>
__global__ __launch_bounds__(BLK) void k_scalar_step_cp(const R* __restrict__ src, R* __restrict__ dst, Fields<R, SEM_SOLID, false, false> f, ScalarArg<R> a,
                                                        int raw, int nxb, int nblocks, R* __restrict__ cp) {
    constexpr int V = 16 / (int)sizeof(R);
    typedef typename VecT<R, V>::type T;
    const Geo& geo = f.geo;
    const int b = xcd_band(blockIdx.x, nblocks);
    const int y = b / nxb;
    const int x0 = ((b % nxb) * BLK + threadIdx.x) * V;
    if (x0 >= geo.nx) return;
    const long long me = geo.at(x0, y);
    const T lk = vload<R, V, false>(f.src + K_LINK * geo.plane + me, true);
    int lw[V], any = 0;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        lw[c] = (int)lk[c];
        any |= lw[c];
    }
    T in[Q], outv[Q];
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        const int cx = raw ? 0 : cxk(k), cy = raw ? 0 : cyk(k);
        in[k] = vload<R, V, NT>(src + k * geo.plane + geo.at(x0 - cx, y + cy), cxk(k) == 0 || raw);
    }
    const bool special = any != 0 || x0 == 0 || x0 + V >= geo.nx || y == 0 || y == geo.ny - 1;
    if (special && !raw) {
        int row[V];
#pragma unroll
        for (int c = 0; c < V; ++c) row[c] = -1;
        if (any & 255) {
            const int32_t* const cr = a.cell_row + (long long)y * geo.nx + x0;
#pragma unroll
            for (int c = 0; c < V; ++c)
                if ((lw[c] & 255) && !(lw[c] & (LINK_SOLID | LINK_HOLD))) row[c] = cr[c];
        }
#pragma unroll
        for (int k = 1; k < Q; ++k) {
            const T own = vload<R, V, NT>(src + opp(k) * geo.plane + me, true);
            const int sy = y + cyk(k);
            const bool out_y = sy < 0 || sy >= geo.ny;
#pragma unroll
            for (int c = 0; c < V; ++c) {
                const int sx = x0 + c - cxk(k);
                if (out_y || sx < 0 || sx >= geo.nx) {
                    in[k][c] = own[c];
                } else if ((lw[c] >> (k - 1)) & 1) {
                    const bool dir = row[c] >= 0 && ((a.bits[row[c]] >> (k - 1)) & 1u);
                    in[k][c] = dir ? a.val[(long long)row[c] * 8 + (k - 1)] - own[c] : own[c];
                }
            }
        }
    }
    T ux, uy, C;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        R u, v, rho;
        f.macro(x0 + c, y, u, v, rho);
        ux[c] = u;
        uy[c] = v;
    }
    scalar_collide<T, R>(in, ux, uy, a.w_plus, a.w_minus, outv, C);
    if (any & LINK_SOLID) {
#pragma unroll
        for (int c = 0; c < V; ++c)
            if (lw[c] & LINK_SOLID) {
#pragma unroll
                for (int k = 0; k < Q; ++k) outv[k][c] = (R)0;
            }
    }
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
    // the C of the collision into the buoyancy plane, zeros on solid lanes (a hold lane stores the sum of what it pulled: a number no
    // flow step uses); the next flow step reads it, so no non-temporal store
#pragma unroll
    for (int c = 0; c < V; ++c)
        if (lw[c] & LINK_SOLID) C[c] = (R)0;
    vstore<R, V, false>(cp + buoy_at(geo, x0, y), C);
}

// The buoyancy plane of a scalar lattice as it is: C as k_scalar_export forms it (the sum of the arriving populations; zeros on solid cells),
// addressed by buoy_at.  After lbm_set_buoyancy, lbm_scalar_begin and lbm_scalar_set_state; every scalar step then keeps it.
template <typename R>
__global__ __launch_bounds__(BLK) void k_scalar_plane(const R* __restrict__ s, const R* __restrict__ links, Geo geo, ScalarArg<R> a, int raw, R* __restrict__ cp) {
    const int x = blockIdx.x * BLK + threadIdx.x, y = blockIdx.y;
    if (x >= geo.nx) return;
    const int lw = (int)links[K_LINK * geo.plane + geo.at(x, y)];
    R g[Q];
    scalar_gather<R>(s, geo, lw, raw, x, y, a, g);
    cp[buoy_at(geo, x, y)] = ((((((((g[0] + g[1]) + g[2]) + g[3]) + g[4]) + g[5]) + g[6]) + g[7]) + g[8]);
}

// Solid cells hold zeros in both scalar lattices: written after every upload, from the link plane of the flow lattice `links`.
template <typename R>
__global__ __launch_bounds__(BLK) void k_scalar_fix(R* __restrict__ a, R* __restrict__ b, const R* __restrict__ links, Geo geo) {
    const int x = blockIdx.x * BLK + threadIdx.x, y = blockIdx.y;
    if (x >= geo.nx) return;
    const long long me = geo.at(x, y);
    if (!((int)links[K_LINK * geo.plane + me] & LINK_SOLID)) return;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        a[k * geo.plane + me] = (R)0;
        b[k * geo.plane + me] = (R)0;
    }
}

// staging [nx][ny] (host layout, the lattice type) -> the buoyancy plane (lbm_set_buoyancy_plane: a checkpoint's)
template <typename R>
__global__ __launch_bounds__(BLK) void k_scalar_plane_import(const R* __restrict__ stage, R* __restrict__ cp, Geo geo) {
    const int x = blockIdx.x * BLK + threadIdx.x, y = blockIdx.y;
    if (x >= geo.nx) return;
    cp[buoy_at(geo, x, y)] = stage[(long long)x * geo.ny + y];
}

// The user's hold cells hold their nine values (scalar_hold_values, rounded once) in both scalar lattices: cell[i] = (x, y), val[i][9].
template <typename R>
__global__ __launch_bounds__(BLK) void k_scalar_hold_fix(R* __restrict__ a, R* __restrict__ b, Geo geo, const int32_t* __restrict__ cell,
                                                         const R* __restrict__ val, int n) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    const long long me = geo.at(cell[2 * i], cell[2 * i + 1]);
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        const R v = val[(long long)i * Q + k];
        a[k * geo.plane + me] = v;
        b[k * geo.plane + me] = v;
    }
}

// staging [9][nx][ny] (host layout) -> scalar lattice, plain populations
template <typename R>
__global__ __launch_bounds__(BLK) void k_scalar_import(const R* __restrict__ stage, R* __restrict__ lat, Geo geo) {
    const int x = blockIdx.x * BLK + threadIdx.x, y = blockIdx.y;
    if (x >= geo.nx) return;
    const long long n = (long long)geo.nx * geo.ny, me = geo.at(x, y);
#pragma unroll
    for (int k = 0; k < Q; ++k) lat[k * geo.plane + me] = stage[k * n + (long long)x * geo.ny + y];
}

// scalar lattice -> staging, in the host layout: the arriving populations (scalar_gather; raw = 1: the stored values as they are) into
// g[9][nx][ny] where g is not null, their sum C (the order of scalar_collide) into conc[nx][ny] where conc is not null.
template <typename R>
__global__ __launch_bounds__(BLK) void k_scalar_export(const R* __restrict__ s, const R* __restrict__ links, Geo geo, ScalarArg<R> a, int raw,
                                                       R* __restrict__ g_out, R* __restrict__ conc) {
    const int x = blockIdx.x * BLK + threadIdx.x, y = blockIdx.y;
    if (x >= geo.nx) return;
    const long long n = (long long)geo.nx * geo.ny, o = (long long)x * geo.ny + y;
    const int lw = (int)links[K_LINK * geo.plane + geo.at(x, y)];
    R g[Q];
    scalar_gather<R>(s, geo, lw, raw, x, y, a, g);
    if (g_out) {
#pragma unroll
        for (int k = 0; k < Q; ++k) g_out[k * n + o] = g[k];
    }
    if (conc) conc[o] = ((((((((g[0] + g[1]) + g[2]) + g[3]) + g[4]) + g[5]) + g[6]) + g[7]) + g[8]);
}

// Totals over the cells that are neither solid nor images of a periodic side: their count, the sum, the minimum and the maximum of C (as
// k_scalar_export forms it) converted to double.  A lane folds its cells in grid-stride order, then the tree of lbm_reduce.hpp.
struct ScalarTotAcc {
    double cells, sum, mn, mx;
    static constexpr int VALS = 4;
    static __device__ __forceinline__ ScalarTotAcc identity() { return ScalarTotAcc{0.0, 0.0, __builtin_huge_val(), -__builtin_huge_val()}; }
    static __device__ __forceinline__ void fold(ScalarTotAcc& a, const ScalarTotAcc& b) {
#pragma clang fp contract(off)
        a.cells = a.cells + b.cells;
        a.sum = a.sum + b.sum;
        a.mn = b.mn < a.mn ? b.mn : a.mn;
        a.mx = b.mx > a.mx ? b.mx : a.mx;
    }
    template <typename F>
    __device__ __forceinline__ void each(F&& f) { f(cells); f(sum); f(mn); f(mx); }
};
constexpr int SCALAR_BLOCKS = 256;   // partial results of the totals

template <typename R>
__global__ __launch_bounds__(BLK) void k_scalar_totals(const R* __restrict__ s, const R* __restrict__ links, Geo geo, ScalarArg<R> a, int raw, int px, int py,
                                                       double* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double shm[BLK / RED_WAVE][ScalarTotAcc::VALS];
    const long long n = (long long)geo.nx * geo.ny;
    ScalarTotAcc acc = ScalarTotAcc::identity();
    for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < n; i += (long long)gridDim.x * BLK) {
        const int y = (int)(i / geo.nx), x = (int)(i - (long long)y * geo.nx);
        const int lw = (int)links[K_LINK * geo.plane + geo.at(x, y)];
        if ((lw & LINK_SOLID) || lbmhost::periodic_image(x, y, geo.nx, geo.ny, px != 0, py != 0)) continue;
        R g[Q];
        scalar_gather<R>(s, geo, lw, raw, x, y, a, g);
        const double C = (double)((((((((g[0] + g[1]) + g[2]) + g[3]) + g[4]) + g[5]) + g[6]) + g[7]) + g[8]);
        ScalarTotAcc::fold(acc, ScalarTotAcc{1.0, C, C, C});
    }
    red_wave(acc);
    if (red_workgroup<ScalarTotAcc, BLK / RED_WAVE>(acc, shm)) red_store(partial + (size_t)blockIdx.x * ScalarTotAcc::VALS, acc);
}
// the final pass, one wave: rec = {step, cells, sum, min, max}
__global__ __launch_bounds__(RED_WAVE) void k_scalar_totals_final(const double* __restrict__ partial, int nper, double step, double* __restrict__ rec) {
    const ScalarTotAcc acc = red_final<ScalarTotAcc>(partial, nper);
    if (threadIdx.x == 0) {
        rec[0] = step;
        red_store(rec + 1, acc);
    }
}

// The scalar that enters the fluid per step through the links of each body: over the flow's link list (lbm_bodies.hpp, one workgroup per
// chunk as k_body_force), links += 1, flux += (double)g_k - (double)own, own = the cell's stored slot opp(k) and g_k what the next gather
// of the cell returns for the link: own on an adiabatic link (the term is an exact zero), t - own on a Dirichlet link.
struct ScalarFluxAcc {
    double links, flux;
    static constexpr int VALS = 2;
    static __device__ __forceinline__ ScalarFluxAcc identity() { return ScalarFluxAcc{0.0, 0.0}; }
    static __device__ __forceinline__ void fold(ScalarFluxAcc& a, const ScalarFluxAcc& b) {
#pragma clang fp contract(off)
        a.links = a.links + b.links;
        a.flux = a.flux + b.flux;
    }
    template <typename F>
    __device__ __forceinline__ void each(F&& f) { f(links); f(flux); }
};
template <typename R>
__global__ __launch_bounds__(BLK) void k_scalar_flux(const R* __restrict__ s, Geo geo, ScalarArg<R> a, const lbmhost::BodyLink* __restrict__ links,
                                                     const lbmhost::BodyChunk* __restrict__ chunks, double* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double shm[BLK / RED_WAVE][ScalarFluxAcc::VALS];
    const lbmhost::BodyChunk ch = chunks[blockIdx.x];
    ScalarFluxAcc acc = ScalarFluxAcc::identity();
    for (int i = threadIdx.x; i < ch.n; i += BLK) {
        const lbmhost::BodyLink l = links[ch.begin + i];
        const int x = l.x, y = l.yk >> 4, k = l.yk & 15;
        const R own = s[opp(k) * geo.plane + geo.at(x, y)];
        const int row = a.cell_row[(long long)y * geo.nx + x];
        const bool dir = row >= 0 && ((a.bits[row] >> (k - 1)) & 1u);
        const R g = dir ? a.val[(long long)row * 8 + (k - 1)] - own : own;
        acc.links = acc.links + 1.0;
        acc.flux = acc.flux + ((double)g - (double)own);
    }
    red_wave(acc);
    if (red_workgroup<ScalarFluxAcc, BLK / RED_WAVE>(acc, shm)) red_store(partial + (size_t)blockIdx.x * ScalarFluxAcc::VALS, acc);
}
// the final pass, one wave per body over the body's chunks: rec[body] = {step, links, flux}
__global__ __launch_bounds__(RED_WAVE) void k_scalar_flux_final(const double* __restrict__ partial, const int32_t* __restrict__ first, double step,
                                                                double* __restrict__ rec) {
    const int body = blockIdx.x;
    const ScalarFluxAcc acc = red_final<ScalarFluxAcc>(partial + (size_t)first[body] * ScalarFluxAcc::VALS, first[body + 1] - first[body]);
    if (threadIdx.x == 0) {
        rec[3 * body] = step;
        red_store(rec + 3 * body + 1, acc);
    }
}
#endif   // __HIPCC__
