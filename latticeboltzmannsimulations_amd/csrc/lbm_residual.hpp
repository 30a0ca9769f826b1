// lbm_residual.hpp -- kernels of the field residual (lbm_residual_*; contract in include/lbm.h): one streaming pass over the lattice
// that forms the macroscopic state k_export_macro would export, compares it with the snapshot of the previous sample, replaces the
// snapshot and reduces the differences to nine numbers per workgroup; a small kernel that folds the workgroups' results, in index
// order, into the record.  The reduction is the monitor's tree (lane, wave-64 shuffles, the workgroup's waves through LDS, one
// partial result per workgroup, no atomics).  Included by lbm_residual.hip alone.
#pragma once
#include "lbm_kernels.hpp"

// What a lane, a wave, a workgroup and the final pass carry: two counts, three sums, the (d2, x, y) maximum (x < 0: none yet) and the
// maximum of dr2.
struct ResAcc {
    double cells, nonfinite, sum_du2, sum_u2, sum_drho2, max_du2;
    int max_x, max_y;
    double max_drho2;
};
constexpr int RES_VALS = 9;          // doubles of one partial result: the members of ResAcc in order
constexpr int RES_WAVE = 64;
constexpr int RES_REC = (int)(sizeof(lbm_residual_record) / sizeof(double));

__device__ __forceinline__ ResAcc res_identity() {
    return ResAcc{0.0, 0.0, 0.0, 0.0, 0.0, -__builtin_inf(), -1, -1, -__builtin_inf()};
}

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

// wave-64 tree through shuffles: lane 0 ends with the wave's result
__device__ __forceinline__ void res_wave_reduce(ResAcc& a) {
#pragma unroll
    for (int off = RES_WAVE / 2; off > 0; off >>= 1) {
        ResAcc b;
        b.cells = __shfl_down(a.cells, off, RES_WAVE);
        b.nonfinite = __shfl_down(a.nonfinite, off, RES_WAVE);
        b.sum_du2 = __shfl_down(a.sum_du2, off, RES_WAVE);
        b.sum_u2 = __shfl_down(a.sum_u2, off, RES_WAVE);
        b.sum_drho2 = __shfl_down(a.sum_drho2, off, RES_WAVE);
        b.max_du2 = __shfl_down(a.max_du2, off, RES_WAVE);
        b.max_x = __shfl_down(a.max_x, off, RES_WAVE);
        b.max_y = __shfl_down(a.max_y, off, RES_WAVE);
        b.max_drho2 = __shfl_down(a.max_drho2, off, RES_WAVE);
        res_fold(a, b);
    }
}

__device__ __forceinline__ void res_store(double* __restrict__ p, const ResAcc& a) {
    p[0] = a.cells; p[1] = a.nonfinite; p[2] = a.sum_du2; p[3] = a.sum_u2; p[4] = a.sum_drho2; p[5] = a.max_du2;
    p[6] = (double)a.max_x; p[7] = (double)a.max_y; p[8] = a.max_drho2;
}
__device__ __forceinline__ ResAcc res_load(const double* __restrict__ p) {
    return ResAcc{p[0], p[1], p[2], p[3], p[4], p[5], (int)p[6], (int)p[7], p[8]};
}

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

// The sample pass: grid-stride over the lane groups of one lattice (blockIdx.z: lattice of the batch); per cell the gather + macros of
// k_export_macro.  Reads the snapshot, writes the current sample over it, reduces; one partial result per workgroup:
// partial[(blockIdx.z * gridDim.x + blockIdx.x) * RES_VALS ...].  No atomics.  Pure streaming: 9 sizeof(R) + 3 sizeof(S) read and
// 3 sizeof(S) written per cell.
template <typename R, typename S, int SEM, bool PROM>
__global__ __launch_bounds__(BLK) void k_residual(const R* __restrict__ src, Geo geo, int raw, R uLB, long long bstride, S* __restrict__ snap,
                                                  double* __restrict__ partial) {
#pragma clang fp contract(off)
    constexpr int CPL = ResGroup<S>::CPL;
    typedef typename ResGroup<S>::vec vec;
    __shared__ double sh[BLK / RES_WAVE][RES_VALS];
    const int nxg = (geo.nx + CPL - 1) / CPL;
    const long long ngroups = (long long)geo.ny * nxg;   // = the elements of one plane / CPL
    src += blockIdx.z * bstride;
    vec* sn = (vec*)snap + blockIdx.z * 3 * ngroups;
    ResAcc a = res_identity();
    for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < ngroups; i += (long long)gridDim.x * BLK) {
        const int y = (int)(i / nxg), x = CPL * (int)(i - (long long)y * nxg), gy = geo.y0 + y;
        const vec pu = sn[i], pv = sn[ngroups + i], pr = sn[2 * ngroups + i];
        vec cu = {}, cv = {}, cr = {};
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            if (x + j >= geo.nx) break;   // (the padding cells of the row's last group)
            R g[Q], rho, ux, uy;
            gather<R, SEM, PROM>(src, geo, raw, uLB, x + j, y, g);
            macros<R, false, SEM>(g, x + j, gy, geo.nx, geo.NY, uLB, rho, ux, uy);
            cu[j] = (S)ux; cv[j] = (S)uy; cr[j] = (S)rho;
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
    res_wave_reduce(a);
    const int wave = threadIdx.x / RES_WAVE;
    if (threadIdx.x % RES_WAVE == 0) res_store(sh[wave], a);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < BLK / RES_WAVE; ++w) res_fold(a, res_load(sh[w]));
        res_store(partial + ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * RES_VALS, a);
    }
}

// The final pass, one wave per lattice: lane l folds the partial results l * chunk .. (l + 1) * chunk - 1 in index order, the lanes
// combine by the same shuffle tree, lane 0 writes the record.  rec: the records of this sample, [batch].
__global__ __launch_bounds__(RES_WAVE) void k_residual_final(const double* __restrict__ partial, int nper, double step, double step_prev,
                                                             double* __restrict__ rec) {
    const int z = blockIdx.x, lane = threadIdx.x;
    partial += (size_t)z * nper * RES_VALS;
    rec += (size_t)z * RES_REC;
    const int chunk = (nper + RES_WAVE - 1) / RES_WAVE;
    ResAcc a = res_identity();
    for (int i = lane * chunk; i < nper && i < (lane + 1) * chunk; ++i) res_fold(a, res_load(partial + (size_t)i * RES_VALS));
    res_wave_reduce(a);
    if (lane == 0) {
        rec[0] = step;
        rec[1] = step_prev;
        res_store(rec + 2, a);
    }
}
