// lbm_monitor.hpp -- kernels of the run monitor (lbm_monitor*, lbm_get_lines; contract in include/lbm.h): one pass over the lattice
// that reduces the macroscopic state k_export_macro would export to ten numbers per workgroup, a small kernel that folds the
// workgroups' results into the record and evaluates the probe cells, and the export of one column and one row.  Included by
// lbm_monitor.hip alone.
#pragma once
#include "lbm_kernels.hpp"

// Window, boxes and probes of lbm_monitor_spec, by value in the kernel arguments.
struct MonSpec {
    int host_f32;                    // round to float before widening (host_dtype = LBM_F32)
    int x_lo, x_hi, y_lo, y_hi;      // y: global rows
    int nboxes, nprobes;
    int box[LBM_MONITOR_MAX_BOXES][4];
    int probe[LBM_MONITOR_MAX_PROBES][2];
};

// What a lane, a wave, a workgroup and the final pass carry: five sums, the maximum and the (q, x, y) minimum (x < 0: none yet).
struct MonAcc {
    double nonfinite, sum_ux, sum_uy, sum_rho, sum_q, max_q, min_q;
    int min_x, min_y;
};
constexpr int MON_VALS = 9;          // doubles of one partial result: the members of MonAcc in order
constexpr int MON_WAVE = 64;
constexpr int MON_REC = (int)(sizeof(lbm_monitor_record) / sizeof(double));

__device__ __forceinline__ MonAcc mon_identity() {
    return MonAcc{0.0, 0.0, 0.0, 0.0, 0.0, -__builtin_inf(), __builtin_inf(), -1, -1};
}

// Is candidate a the minimum rather than b?  Explicitly on (q, x, y): the device visits the cells x fastest, np.nanargmin on the
// [X][Y] host array y fastest, so "first seen" would pick another cell among equal q.
__device__ __forceinline__ bool mon_before(double qa, int xa, int ya, double qb, int xb, int yb) {
    // (one branch-free predicate; the callers take q, x and y by selects on its result, mon_take)
    return (xa >= 0) & ((xb < 0) | (qa < qb) | ((qa == qb) & ((xa < xb) | ((xa == xb) & (ya < yb)))));
}
__device__ __forceinline__ void mon_take(bool take, double& q, int& x, int& y, double qb, int xb, int yb) {
    q = take ? qb : q;
    x = take ? xb : x;
    y = take ? yb : y;
}

// a := a (+) b, the one combining step of every level of the tree (sums: a + b in this order)
__device__ __forceinline__ void mon_fold(MonAcc& a, const MonAcc& b) {
#pragma clang fp contract(off)
    a.nonfinite = a.nonfinite + b.nonfinite;
    a.sum_ux = a.sum_ux + b.sum_ux;
    a.sum_uy = a.sum_uy + b.sum_uy;
    a.sum_rho = a.sum_rho + b.sum_rho;
    a.sum_q = a.sum_q + b.sum_q;
    a.max_q = b.max_q > a.max_q ? b.max_q : a.max_q;
    mon_take(mon_before(b.min_q, b.min_x, b.min_y, a.min_q, a.min_x, a.min_y), a.min_q, a.min_x, a.min_y, b.min_q, b.min_x, b.min_y);
}

// wave-64 tree through shuffles: lane 0 ends with the wave's result
__device__ __forceinline__ void mon_wave_reduce(MonAcc& a) {
#pragma unroll
    for (int off = MON_WAVE / 2; off > 0; off >>= 1) {
        MonAcc b;
        b.nonfinite = __shfl_down(a.nonfinite, off, MON_WAVE);
        b.sum_ux = __shfl_down(a.sum_ux, off, MON_WAVE);
        b.sum_uy = __shfl_down(a.sum_uy, off, MON_WAVE);
        b.sum_rho = __shfl_down(a.sum_rho, off, MON_WAVE);
        b.sum_q = __shfl_down(a.sum_q, off, MON_WAVE);
        b.max_q = __shfl_down(a.max_q, off, MON_WAVE);
        b.min_q = __shfl_down(a.min_q, off, MON_WAVE);
        b.min_x = __shfl_down(a.min_x, off, MON_WAVE);
        b.min_y = __shfl_down(a.min_y, off, MON_WAVE);
        mon_fold(a, b);
    }
}

__device__ __forceinline__ void mon_store(double* __restrict__ p, const MonAcc& a) {
    p[0] = a.nonfinite; p[1] = a.sum_ux; p[2] = a.sum_uy; p[3] = a.sum_rho; p[4] = a.sum_q; p[5] = a.max_q; p[6] = a.min_q;
    p[7] = (double)a.min_x; p[8] = (double)a.min_y;
}
__device__ __forceinline__ MonAcc mon_load(const double* __restrict__ p) {
    return MonAcc{p[0], p[1], p[2], p[3], p[4], p[5], p[6], (int)p[7], (int)p[8]};
}

// the value lbm_get_fields(host_dtype) would hand out, as a double
template <typename R>
__device__ __forceinline__ double mon_value(R v, int host_f32) { return host_f32 ? (double)(float)v : (double)v; }

// The fused monitor pass: grid-stride over the cells of one lattice (blockIdx.z: lattice of the batch), x fastest; per cell the gather +
// macros of k_export_macro.  Lanes reduce by wave-64 shuffles, the workgroup's four waves through 4 x MON_VALS doubles of LDS; one
// partial result per workgroup: partial[(blockIdx.z * gridDim.x + blockIdx.x) * MON_VALS ...].  No atomics.  Reads the nine planes
// once, like k_reduce_u.
template <typename R, int SEM, bool PROM>
__global__ __launch_bounds__(BLK) void k_monitor(const R* __restrict__ src, Geo geo, int raw, R uLB, double den, long long bstride, MonSpec sp,
                                                 double* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double sh[BLK / MON_WAVE][MON_VALS];
    src += blockIdx.z * bstride;
    const long long n = (long long)geo.nx * geo.ny;
    MonAcc a = mon_identity();
    for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < n; i += (long long)gridDim.x * BLK) {
        const int y = (int)(i / geo.nx), x = (int)(i - (long long)y * geo.nx), gy = geo.y0 + y;
        R g[Q], rho, ux, uy;
        gather<R, SEM, PROM>(src, geo, raw, uLB, x, y, g);
        macros<R, false, SEM>(g, x, gy, geo.nx, geo.NY, uLB, rho, ux, uy);
        const double dx = mon_value(ux, sp.host_f32), dy = mon_value(uy, sp.host_f32), dr = mon_value(rho, sp.host_f32);
        if (!(__builtin_isfinite(dx) && __builtin_isfinite(dy) && __builtin_isfinite(dr))) {
            a.nonfinite = a.nonfinite + 1.0;
            continue;
        }
        const double xx = dx * dx, yy = dy * dy;
        const double q = (xx + yy) / den;
        a.sum_ux = a.sum_ux + dx;
        a.sum_uy = a.sum_uy + dy;
        a.sum_rho = a.sum_rho + dr;
        a.sum_q = a.sum_q + q;
        a.max_q = q > a.max_q ? q : a.max_q;
        bool in = x >= sp.x_lo && x < sp.x_hi && gy >= sp.y_lo && gy < sp.y_hi;
        for (int b = 0; b < sp.nboxes; ++b)
            in = in && !(x >= sp.box[b][0] && x < sp.box[b][1] && gy >= sp.box[b][2] && gy < sp.box[b][3]);
        mon_take(in & mon_before(q, x, gy, a.min_q, a.min_x, a.min_y), a.min_q, a.min_x, a.min_y, q, x, gy);
    }
    mon_wave_reduce(a);
    const int wave = threadIdx.x / MON_WAVE;
    if (threadIdx.x % MON_WAVE == 0) mon_store(sh[wave], a);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < BLK / MON_WAVE; ++w) mon_fold(a, mon_load(sh[w]));
        mon_store(partial + ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * MON_VALS, a);
    }
}

// The final pass, one wave per lattice: lane l folds the partial results l * chunk .. (l + 1) * chunk - 1 in index order, the lanes
// combine by the same shuffle tree, lane 0 writes the record; lanes 0 .. 7 evaluate the probe cells (gather + macros of the one cell).
// rec: the records of this sample, [batch].
template <typename R, int SEM, bool PROM>
__global__ __launch_bounds__(MON_WAVE) void k_monitor_final(const double* __restrict__ partial, int nper, const R* __restrict__ src, Geo geo, int raw,
                                                            R uLB, long long bstride, MonSpec sp, double step, double* __restrict__ rec) {
    const int z = blockIdx.x, lane = threadIdx.x;
    src += z * bstride;
    partial += (size_t)z * nper * MON_VALS;
    rec += (size_t)z * MON_REC;
    const int chunk = (nper + MON_WAVE - 1) / MON_WAVE;
    MonAcc a = mon_identity();
    for (int i = lane * chunk; i < nper && i < (lane + 1) * chunk; ++i) mon_fold(a, mon_load(partial + (size_t)i * MON_VALS));
    mon_wave_reduce(a);
    if (lane == 0) {
        rec[0] = step;
        mon_store(rec + 1, a);
    }
    if (lane < LBM_MONITOR_MAX_PROBES) {
        double v[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
        if (lane < sp.nprobes) {
            const int x = sp.probe[lane][0], y = sp.probe[lane][1] - geo.y0;
            if (y >= 0 && y < geo.ny) {
                R g[Q], rho, ux, uy;
                gather<R, SEM, PROM>(src, geo, raw, uLB, x, y, g);
                macros<R, false, SEM>(g, x, geo.y0 + y, geo.nx, geo.NY, uLB, rho, ux, uy);
                v[0] = mon_value(ux, sp.host_f32); v[1] = mon_value(uy, sp.host_f32); v[2] = mon_value(rho, sp.host_f32);
            }
        }
        double* p = rec + 1 + MON_VALS + 3 * lane;
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
    }
}

// Column x (all local rows) and local row ly (ly < 0: none) of the macroscopic state k_export_macro would export, in host layout:
// stage of lattice z = [ux | uy | rho][ny] of the column, then [ux | uy | rho][nx] of the row.  One thread per cell of either line.
template <typename R, int SEM, bool PROM>
__global__ __launch_bounds__(BLK) void k_export_lines(const R* __restrict__ src, Geo geo, int raw, R uLB, long long bstride, int cx, int ly,
                                                      R* __restrict__ stage) {
    src += blockIdx.z * bstride;
    stage += (size_t)blockIdx.z * 3 * (geo.ny + geo.nx);
    const int t = blockIdx.x * BLK + threadIdx.x;
    int x, y;
    R* out;
    int n;
    if (t < geo.ny) {
        if (cx < 0) return;
        x = cx; y = t; out = stage + t; n = geo.ny;
    } else if (t < geo.ny + geo.nx) {
        if (ly < 0) return;
        x = t - geo.ny; y = ly; out = stage + 3 * geo.ny + x; n = geo.nx;
    } else {
        return;
    }
    R g[Q], rho, ux, uy;
    gather<R, SEM, PROM>(src, geo, raw, uLB, x, y, g);
    macros<R, false, SEM>(g, x, geo.y0 + y, geo.nx, geo.NY, uLB, rho, ux, uy);
    out[0] = ux; out[n] = uy; out[2 * n] = rho;
}
