// lbm_monitor.hpp -- kernels of the run monitor (lbm_monitor*, lbm_get_lines; contract in include/lbm.h): one pass over the lattice
// that reduces the exported state (the view of lbm_fields.hpp) to ten numbers per workgroup, a small kernel that folds the
// workgroups' results into the record and evaluates the probe cells, and the export of one column and one row.  Included by
// lbm_monitor.hip alone.
#pragma once
#include "lbm_fields.hpp"
#include "lbm_reduce.hpp"

// Window, boxes and probes of lbm_monitor_spec, by value in the kernel arguments.
struct MonSpec {
    int host_f32;                    // round to float before widening (host_dtype = LBM_F32)
    int x_lo, x_hi, y_lo, y_hi;      // y: global rows
    int nboxes, nprobes;
    int box[LBM_MONITOR_MAX_BOXES][4];
    int probe[LBM_MONITOR_MAX_PROBES][2];
};

// What a lane, a wave, a workgroup and the final pass carry (an accumulator of lbm_reduce.hpp): five sums, the maximum and the
// (q, x, y) minimum (x < 0: none yet).
struct MonAcc {
    double nonfinite, sum_ux, sum_uy, sum_rho, sum_q, max_q, min_q;
    int min_x, min_y;
    static constexpr int VALS = 9;
    static __device__ __forceinline__ MonAcc identity() { return MonAcc{0.0, 0.0, 0.0, 0.0, 0.0, -__builtin_inf(), __builtin_inf(), -1, -1}; }
    static __device__ __forceinline__ void fold(MonAcc& a, const MonAcc& b);   // = mon_fold
    template <typename F>
    __device__ __forceinline__ void each(F&& f) {
        f(nonfinite); f(sum_ux); f(sum_uy); f(sum_rho); f(sum_q); f(max_q); f(min_q); f(min_x); f(min_y);
    }
};
constexpr int MON_VALS = MonAcc::VALS;   // doubles of one partial result: the members of MonAcc in order
constexpr int MON_REC = (int)(sizeof(lbm_monitor_record) / sizeof(double));

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

__device__ __forceinline__ void MonAcc::fold(MonAcc& a, const MonAcc& b) { mon_fold(a, b); }

// The fused monitor pass: grid-stride over the cells of one lattice (blockIdx.z: lattice of the batch), x fastest; per cell the
// exported values of the view.  The tree of lbm_reduce.hpp leaves one partial result per workgroup:
// partial[(blockIdx.z * gridDim.x + blockIdx.x) * MON_VALS ...].  Reads the nine planes once, like k_reduce_u.
template <typename R, int SEM, bool PROM, bool SHAPE = false>
__global__ __launch_bounds__(BLK) void k_monitor(Fields<R, SEM, PROM, SHAPE> f, double den, MonSpec sp, double* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double sh[BLK / RED_WAVE][MON_VALS];
    const Geo& geo = f.geo;
    const auto lat = f.lattice(blockIdx.z);
    const long long n = (long long)geo.nx * geo.ny;
    MonAcc a = MonAcc::identity();
    for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < n; i += (long long)gridDim.x * BLK) {
        const int y = (int)(i / geo.nx), x = (int)(i - (long long)y * geo.nx), gy = geo.y0 + y;
        R rho, ux, uy;   // (Fields::exported spelled out: through it this loop came out 21 instructions longer)
        lat.macro(x, y, ux, uy, rho);
        const double dx = as_exported(ux, sp.host_f32), dy = as_exported(uy, sp.host_f32), dr = as_exported(rho, sp.host_f32);
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
    red_wave(a);
    if (red_workgroup<MonAcc, BLK / RED_WAVE>(a, sh)) red_store(partial + ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * MON_VALS, a);
}

// The final pass, one wave per lattice (red_final): lane 0 writes the record; lanes 0 .. 7 evaluate the probe cells (the exported
// values of the one cell).  rec: the records of this sample, [batch].
template <typename R, int SEM, bool PROM, bool SHAPE = false>
__global__ __launch_bounds__(RED_WAVE) void k_monitor_final(const double* __restrict__ partial, int nper, Fields<R, SEM, PROM, SHAPE> f, MonSpec sp, double step,
                                                            double* __restrict__ rec) {
    const int z = blockIdx.x, lane = threadIdx.x;
    rec += (size_t)z * MON_REC;
    const MonAcc a = red_final<MonAcc>(partial + (size_t)z * nper * MON_VALS, nper);
    if (lane == 0) {
        rec[0] = step;
        red_store(rec + 1, a);
    }
    if (lane < LBM_MONITOR_MAX_PROBES) {
        double v[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
        if (lane < sp.nprobes) {
            const int x = sp.probe[lane][0], y = sp.probe[lane][1] - f.geo.y0;
            if (y >= 0 && y < f.geo.ny) f.lattice(z).exported(x, y, sp.host_f32, v[0], v[1], v[2]);
        }
        double* p = rec + 1 + MON_VALS + 3 * lane;
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
    }
}

// Column x (all local rows) and local row ly (ly < 0: none) of the exported state, in host layout:
// stage of lattice z = [ux | uy | rho][ny] of the column, then [ux | uy | rho][nx] of the row.  One thread per cell of either line.
template <typename R, int SEM, bool PROM, bool SHAPE = false>
__global__ __launch_bounds__(BLK) void k_export_lines(Fields<R, SEM, PROM, SHAPE> f, int cx, int ly, R* __restrict__ stage) {
    const Geo& geo = f.geo;
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
    R rho, ux, uy;
    f.lattice(blockIdx.z).macro(x, y, ux, uy, rho);
    out[0] = ux; out[n] = uy; out[2 * n] = rho;
}
