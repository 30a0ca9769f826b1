// lbm_residual.hpp -- kernels of the field residual (lbm_residual_*; contract in include/lbm.h): one streaming pass over the lattice
// that forms the exported state (the view of lbm_fields.hpp), compares it with the snapshot of the previous sample, replaces the
// snapshot and reduces the differences to nine numbers per workgroup; a small kernel that folds the workgroups' results, in index
// order, into the record.  The reduction is the tree of lbm_reduce.hpp.  Included by lbm_residual.hip alone.
#pragma once
#include "lbm_fields.hpp"
#include "lbm_reduce.hpp"

// What a lane, a wave, a workgroup and the final pass carry (an accumulator of lbm_reduce.hpp): two counts, three sums, the
// (d2, x, y) maximum (x < 0: none yet) and the maximum of dr2.
struct ResAcc {
    double cells, nonfinite, sum_du2, sum_u2, sum_drho2, max_du2;
    int max_x, max_y;
    double max_drho2;
    static constexpr int VALS = 9;
    static __device__ __forceinline__ ResAcc identity() { return ResAcc{0.0, 0.0, 0.0, 0.0, 0.0, -__builtin_inf(), -1, -1, -__builtin_inf()}; }
    static __device__ __forceinline__ void fold(ResAcc& a, const ResAcc& b);   // = res_fold
    template <typename F>
    __device__ __forceinline__ void each(F&& f) {
        f(cells); f(nonfinite); f(sum_du2); f(sum_u2); f(sum_drho2); f(max_du2); f(max_x); f(max_y); f(max_drho2);
    }
};
constexpr int RES_VALS = ResAcc::VALS;   // doubles of one partial result: the members of ResAcc in order
constexpr int RES_REC = (int)(sizeof(lbm_residual_record) / sizeof(double));

// Is candidate a the maximum rather than b?  Explicitly on (d2, x, y): the larger d2, then the smaller x, then the smaller y -- the
// first hit of np.argmax on the [X][Y] host array, whatever order the device visits the cells in.
__device__ __forceinline__ bool res_before(double qa, int xa, int ya, double qb, int xb, int yb) {
    return (xa >= 0) & ((xb < 0) | (qa > qb) | ((qa == qb) & ((xa < xb) | ((xa == xb) & (ya < yb)))));
}

// a := a (+) b, the one combining step of every level of the tree (sums: a + b in this order)
__device__ __forceinline__ void res_fold(ResAcc& a, const ResAcc& b) {
#pragma clang fp contract(off)
    a.cells = a.cells + b.cells;
    a.nonfinite = a.nonfinite + b.nonfinite;
    a.sum_du2 = a.sum_du2 + b.sum_du2;
    a.sum_u2 = a.sum_u2 + b.sum_u2;
    a.sum_drho2 = a.sum_drho2 + b.sum_drho2;
    const bool take = res_before(b.max_du2, b.max_x, b.max_y, a.max_du2, a.max_x, a.max_y);
    a.max_du2 = take ? b.max_du2 : a.max_du2;
    a.max_x = take ? b.max_x : a.max_x;
    a.max_y = take ? b.max_y : a.max_y;
    a.max_drho2 = b.max_drho2 > a.max_drho2 ? b.max_drho2 : a.max_drho2;
}

__device__ __forceinline__ void ResAcc::fold(ResAcc& a, const ResAcc& b) { res_fold(a, b); }

// The snapshot: three planes [ux | uy | rho] per lattice, each [ny_local][nxa], x fastest, nxa = nx rounded up to a whole number of
// lane groups; element type S = the type lbm_get_fields(host_dtype) hands out (float unless lattice and host_dtype are both double), so
// that storing a sample value IS the rounding to host_dtype and keeps its bits, whatever they are.  One lane owns the CPL = 16 / sizeof(S)
// neighbouring cells of one group: every access to the snapshot is 16 B per lane and coalesced along x (the padding cells of the last
// group of a row hold 0 and take no part).
template <typename S>
struct ResGroup {
    static constexpr int CPL = 16 / (int)sizeof(S);
    typedef S vec __attribute__((ext_vector_type(CPL)));
};

// The sample pass: grid-stride over the lane groups of one lattice (blockIdx.z: lattice of the batch); per cell the macroscopic
// state of the view.  Reads the snapshot, writes the current sample over it, reduces; one partial result per workgroup:
// partial[(blockIdx.z * gridDim.x + blockIdx.x) * RES_VALS ...].  No atomics.  Pure streaming: 9 sizeof(R) + 3 sizeof(S) read and
// 3 sizeof(S) written per cell.
template <typename R, typename S, int SEM, bool PROM, bool SHAPE = false>
__global__ __launch_bounds__(BLK) void k_residual(Fields<R, SEM, PROM, SHAPE> f, S* __restrict__ snap, double* __restrict__ partial) {
#pragma clang fp contract(off)
    constexpr int CPL = ResGroup<S>::CPL;
    typedef typename ResGroup<S>::vec vec;
    __shared__ double sh[BLK / RED_WAVE][RES_VALS];
    const Geo& geo = f.geo;
    const int nxg = (geo.nx + CPL - 1) / CPL;
    const long long ngroups = (long long)geo.ny * nxg;   // = the elements of one plane / CPL
    const auto lat = f.lattice(blockIdx.z);
    vec* sn = (vec*)snap + blockIdx.z * 3 * ngroups;
    ResAcc a = ResAcc::identity();
    for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < ngroups; i += (long long)gridDim.x * BLK) {
        const int y = (int)(i / nxg), x = CPL * (int)(i - (long long)y * nxg), gy = geo.y0 + y;
        const vec pu = sn[i], pv = sn[ngroups + i], pr = sn[2 * ngroups + i];
        vec cu = {}, cv = {}, cr = {};
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            if (x + j >= geo.nx) break;   // (the padding cells of the row's last group)
            R rho, ux, uy;
            lat.macro(x + j, y, ux, uy, rho);
            cu[j] = (S)ux; cv[j] = (S)uy; cr[j] = (S)rho;   // (storing through S is the rounding of Fields::exported, see ResGroup)
            const double dux_now = (double)cu[j], duy_now = (double)cv[j], drho_now = (double)cr[j];
            const double pux = (double)pu[j], puy = (double)pv[j], prho = (double)pr[j];
            const bool fin = __builtin_isfinite(dux_now) && __builtin_isfinite(duy_now) && __builtin_isfinite(drho_now) &&
                             __builtin_isfinite(pux) && __builtin_isfinite(puy) && __builtin_isfinite(prho);
            if (!fin) {
                a.nonfinite = a.nonfinite + 1.0;
                continue;
            }
            const double dux = dux_now - pux, duy = duy_now - puy, dr = drho_now - prho;
            const double dxx = dux * dux, dyy = duy * duy;
            const double d2 = dxx + dyy;
            const double uxx = dux_now * dux_now, uyy = duy_now * duy_now;
            const double u2 = uxx + uyy;
            const double dr2 = dr * dr;
            a.cells = a.cells + 1.0;
            a.sum_du2 = a.sum_du2 + d2;
            a.sum_u2 = a.sum_u2 + u2;
            a.sum_drho2 = a.sum_drho2 + dr2;
            const bool take = res_before(d2, x + j, gy, a.max_du2, a.max_x, a.max_y);
            a.max_du2 = take ? d2 : a.max_du2;
            a.max_x = take ? x + j : a.max_x;
            a.max_y = take ? gy : a.max_y;
            a.max_drho2 = dr2 > a.max_drho2 ? dr2 : a.max_drho2;
        }
        sn[i] = cu; sn[ngroups + i] = cv; sn[2 * ngroups + i] = cr;
    }
    red_wave(a);
    if (red_workgroup<ResAcc, BLK / RED_WAVE>(a, sh)) red_store(partial + ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * RES_VALS, a);
}

// The final pass, one wave per lattice (red_final): lane 0 writes the record.  rec: the records of this sample, [batch].
__global__ __launch_bounds__(RED_WAVE) void k_residual_final(const double* __restrict__ partial, int nper, double step, double step_prev,
                                                             double* __restrict__ rec) {
    const int z = blockIdx.x;
    rec += (size_t)z * RES_REC;
    const ResAcc a = red_final<ResAcc>(partial + (size_t)z * nper * RES_VALS, nper);
    if (threadIdx.x == 0) {
        rec[0] = step;
        rec[1] = step_prev;
        red_store(rec + 2, a);
    }
}
