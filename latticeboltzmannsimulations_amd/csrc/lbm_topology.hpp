// lbm_topology.hpp -- kernels of the flow topology (lbm_topology, lbm_get_stream_function; contract in include/lbm.h): the stream
// function psi as a two-level prefix sum along x, its extrema inside up to eight windows, the vorticity omega.  The sample is the
// monitor's (Fields::exported, lbm_fields.hpp).  Included by lbm_topology.hip alone.
//
//   k_topo_totals    a workgroup takes TOPO_ROWS rows x one block of LBM_TOPOLOGY_BLOCK cells of x, plus the cell to its left: the
//                    gather runs along x (coalesced), uy goes to LDS as doubles, one thread per row sums the block's terms in order
//   k_topo_offsets   one thread per row: the exclusive scan of the row's block totals, in order, and |psi| at the right wall
//   k_topo_extrema   the same tile and the same in-order sums, psi = -(off + within); per window the candidates go through the tree of
//                    lbm_reduce.hpp to one partial result per workgroup; FIELDS: psi leaves the tile in host layout
//   k_topo_final     one workgroup per (window, lattice) folds the partial results and evaluates omega at the two extrema
//   k_topo_omega     the omega field from the staged u of the export path, one thread per cell
// Minimum and maximum are taken by a total order on (psi, x, y), so no result depends on the shape of a tree or on scheduling.
#pragma once
#include "lbm_monitor.hpp"

constexpr int TOPO_W = LBM_TOPOLOGY_BLOCK;     // cells of x per block of the prefix sum
constexpr int TOPO_ROWS = 32;                  // rows per tile
constexpr int TOPO_PITCH = TOPO_W + 1;         // doubles per tile row in LDS: the left neighbour + the block; odd, so that the threads
                                               // of phase 2 (one per row) read 32 distinct bank pairs (130 r mod 64 = 2 r)
constexpr int TOPO_PART = 6;                   // doubles of one partial result: min (psi, x, y), max (psi, x, y)
constexpr int TOPO_REC = (int)(sizeof(lbm_topology_record) / sizeof(double));
static_assert(BLK == 4 * TOPO_W && BLK % TOPO_ROWS == 0, "tile mapping");

struct TopoSpec {
    int host_f32;
    int nwindows;
    int win[LBM_TOPOLOGY_MAX_WINDOWS][4];      // x_lo, x_hi, y_lo, y_hi
};

// A candidate extremum: x < 0 = none yet.
struct TopoCand {
    double psi;
    int x, y;
};

// Is candidate a the minimum (MAX: the maximum) rather than b?  Explicitly on (psi, x, y), ties to the smaller x, then the smaller y,
// for both -- like mon_before.
template <bool MAX>
__device__ __forceinline__ bool topo_before(const TopoCand& a, const TopoCand& b) {
    const bool better = MAX ? a.psi > b.psi : a.psi < b.psi;
    return (a.x >= 0) & ((b.x < 0) | better | ((a.psi == b.psi) & ((a.x < b.x) | ((a.x == b.x) & (a.y < b.y)))));
}
template <bool MAX>
__device__ __forceinline__ void topo_fold(TopoCand& a, const TopoCand& b) {
    const bool take = topo_before<MAX>(b, a);
    a.psi = take ? b.psi : a.psi;
    a.x = take ? b.x : a.x;
    a.y = take ? b.y : a.y;
}
__device__ __forceinline__ TopoCand topo_none(bool max) { return TopoCand{max ? -__builtin_inf() : __builtin_inf(), -1, -1}; }

// The minimum and the maximum side by side, an accumulator of lbm_reduce.hpp: the six doubles of a partial result.
struct TopoPair {
    TopoCand lo, hi;
    static constexpr int VALS = TOPO_PART;
    static __device__ __forceinline__ TopoPair identity() { return TopoPair{topo_none(false), topo_none(true)}; }
    static __device__ __forceinline__ void fold(TopoPair& a, const TopoPair& b) {
        topo_fold<false>(a.lo, b.lo);
        topo_fold<true>(a.hi, b.hi);
    }
    template <typename F>
    __device__ __forceinline__ void each(F&& f) {
        f(lo.psi); f(lo.x); f(lo.y); f(hi.psi); f(hi.x); f(hi.y);
    }
};

// ux, uy of cell (x, y) of the view's lattice as lbm_get_fields(host_dtype) hands them out, in double
template <typename F>
__device__ __forceinline__ void topo_u(const F& lat, int host_f32, int x, int y, double& dux, double& duy) {
    double drho;
    lat.exported(x, y, host_f32, dux, duy, drho);
}

// d/di of a line of n >= 2 values at index i from lo = v[i - 1], mid = v[i], hi = v[i + 1] (the one outside the line is not used):
// central inside, one-sided at either end.  The one spelling for the omega field and for omega at an extremum.
__device__ __forceinline__ double topo_diff(double lo, double mid, double hi, int i, int n) {
#pragma clang fp contract(off)
    return i == 0 ? hi - mid : (i == n - 1 ? mid - lo : 0.5 * (hi - lo));
}

// Phase 1 of a tile: uy of rows ty0 .. ty0 + TOPO_ROWS - 1, cells x0 - 1 .. x0 + TOPO_W - 1 into u[r][j] (j = 0: the left neighbour);
// cells outside the lattice are left alone (phase 2 does not read them).
template <typename F>
__device__ __forceinline__ void topo_tile_load(const F& lat, int host_f32, int x0, int ty0, double (*u)[TOPO_PITCH]) {
    const Geo& geo = lat.geo;
    const int lane = threadIdx.x % TOPO_W;
    for (int r = threadIdx.x / TOPO_W; r < TOPO_ROWS; r += BLK / TOPO_W) {
        const int x = x0 + lane, y = ty0 + r;
        if (x < geo.nx && y < geo.ny) {
            double dux, duy;
            topo_u(lat, host_f32, x, y, dux, duy);
            u[r][lane + 1] = duy;
        }
    }
    if (threadIdx.x < TOPO_ROWS && x0 > 0 && ty0 + (int)threadIdx.x < geo.ny) {
        double dux, duy;
        topo_u(lat, host_f32, x0 - 1, ty0 + threadIdx.x, dux, duy);
        u[threadIdx.x][0] = duy;
    }
}

// Phase 2, one thread per row: the running sum of the block's terms t[x] = 0.5 (uy[x - 1] + uy[x]) (t[0] = 0), strictly left to right,
// starting as the first term; returns the last.  STORE: u[r][j] := -(off + within[x0 + j]) for the cells of the block (the slot of the
// left neighbour of cell j, which is read before it is written).
template <bool STORE>
__device__ __forceinline__ double topo_tile_scan(double* __restrict__ u, int x0, int w, double off) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int j = 0; j < w; ++j) {
        const double t = x0 + j == 0 ? 0.0 : 0.5 * (u[j] + u[j + 1]);
        acc = j == 0 ? t : acc + t;
        if (STORE) u[j] = -(off + acc);
    }
    return acc;
}

// total[(z * nb + b) * ny + y] = the sum of the terms of block b of row y.  Grid (nb, tiles of rows, batch).
template <typename R, int SEM, bool PROM, bool SHAPE = false>
__global__ __launch_bounds__(BLK) void k_topo_totals(Fields<R, SEM, PROM, SHAPE> f, int host_f32, double* __restrict__ total) {
    __shared__ double u[TOPO_ROWS][TOPO_PITCH];
    const Geo& geo = f.geo;
    const int x0 = blockIdx.x * TOPO_W, ty0 = blockIdx.y * TOPO_ROWS;
    topo_tile_load(f.lattice(blockIdx.z), host_f32, x0, ty0, u);
    __syncthreads();
    const int y = ty0 + threadIdx.x;
    if (threadIdx.x < TOPO_ROWS && y < geo.ny)
        total[((size_t)blockIdx.z * gridDim.x + blockIdx.x) * geo.ny + y] = topo_tile_scan<false>(u[threadIdx.x], x0, min(TOPO_W, geo.nx - x0), 0.0);
}

// In place: total[z][b][y] becomes off[b] (off[0] = 0, off[b + 1] = off[b] + total[b], in order); close[z * ny + y] = |psi[nx - 1][y]|,
// psi there being -(off[nb - 1] + total[nb - 1]).  One thread per row.
__global__ __launch_bounds__(BLK) void k_topo_offsets(double* __restrict__ total, int nb, int ny, double* __restrict__ close) {
#pragma clang fp contract(off)
    const int y = blockIdx.x * BLK + threadIdx.x;
    if (y >= ny) return;
    double* t = total + (size_t)blockIdx.z * nb * ny + y;
    double off = 0.0;
    for (int b = 0; b < nb; ++b) {
        const double s = t[(size_t)b * ny];
        t[(size_t)b * ny] = off;
        off = off + s;
    }
    close[(size_t)blockIdx.z * ny + y] = __builtin_fabs(off);
}

// psi of the tile, then per window of the spec the extrema over the tile's cells with a finite psi inside it:
// partial[((z * MAX_WINDOWS + w) * nwg + wg) * TOPO_PART ...], wg = blockIdx.y * gridDim.x + blockIdx.x.  FIELDS: psi also goes to
// psi_out[z][nx][ny] (host layout, written along y).
template <typename R, int SEM, bool PROM, bool FIELDS, bool SHAPE = false>
__global__ __launch_bounds__(BLK) void k_topo_extrema(Fields<R, SEM, PROM, SHAPE> f, TopoSpec sp, const double* __restrict__ offs, double* __restrict__ partial,
                                                     double* __restrict__ psi_out) {
    __shared__ double u[TOPO_ROWS][TOPO_PITCH];
    __shared__ double sh[BLK / RED_WAVE][TOPO_PART];
    const Geo& geo = f.geo;
    const int x0 = blockIdx.x * TOPO_W, ty0 = blockIdx.y * TOPO_ROWS, w = min(TOPO_W, geo.nx - x0), h = min(TOPO_ROWS, geo.ny - ty0);
    topo_tile_load(f.lattice(blockIdx.z), sp.host_f32, x0, ty0, u);
    __syncthreads();
    if ((int)threadIdx.x < h)
        topo_tile_scan<true>(u[threadIdx.x], x0, w, offs[((size_t)blockIdx.z * gridDim.x + blockIdx.x) * geo.ny + ty0 + threadIdx.x]);
    __syncthreads();
    if (FIELDS) {
        psi_out += (size_t)blockIdx.z * geo.nx * geo.ny;
        const int r = threadIdx.x % TOPO_ROWS;
        if (r < h)
            for (int j = threadIdx.x / TOPO_ROWS; j < w; j += BLK / TOPO_ROWS) psi_out[(size_t)(x0 + j) * geo.ny + ty0 + r] = u[r][j];
    }
    const int nwg = gridDim.x * gridDim.y, wg = blockIdx.y * gridDim.x + blockIdx.x;
    for (int i = 0; i < sp.nwindows; ++i) {   // (uniform: every thread of the workgroup takes the same trips)
        const int xa = max(sp.win[i][0], x0), xb = min(sp.win[i][1], x0 + w), ya = max(sp.win[i][2], ty0), yb = min(sp.win[i][3], ty0 + h);
        TopoPair e = TopoPair::identity();
        if (xa < xb && ya < yb) {
            for (int t = threadIdx.x; t < TOPO_ROWS * TOPO_W; t += BLK) {
                const int r = t / TOPO_W, j = t % TOPO_W, x = x0 + j, y = ty0 + r;
                if (x < xa || x >= xb || y < ya || y >= yb) continue;
                const TopoCand c{u[r][j], x, y};
                if (!__builtin_isfinite(c.psi)) continue;
                TopoPair::fold(e, TopoPair{c, c});
            }
            red_wave(e);
        }
        if (red_workgroup<TopoPair, BLK / RED_WAVE>(e, sh))
            red_store(partial + (((size_t)blockIdx.z * LBM_TOPOLOGY_MAX_WINDOWS + i) * nwg + wg) * TOPO_PART, e);
        __syncthreads();
    }
}

// omega of cell (x, y) from the cells around it
template <typename F>
__device__ __forceinline__ double topo_omega_at(const F& lat, int host_f32, int x, int y) {
#pragma clang fp contract(off)
    const Geo& geo = lat.geo;
    double ux0, uy0, d, vl = 0.0, vr = 0.0, ul = 0.0, ur = 0.0;
    topo_u(lat, host_f32, x, y, ux0, uy0);
    if (x > 0) topo_u(lat, host_f32, x - 1, y, d, vl);
    if (x < geo.nx - 1) topo_u(lat, host_f32, x + 1, y, d, vr);
    if (y > 0) topo_u(lat, host_f32, x, y - 1, ul, d);
    if (y < geo.ny - 1) topo_u(lat, host_f32, x, y + 1, ur, d);
    const double dvdx = topo_diff(vl, uy0, vr, x, geo.nx), dudy = topo_diff(ul, ux0, ur, y, geo.ny);
    return dvdx + dudy;
}

// One workgroup per (window blockIdx.x, lattice blockIdx.y): folds the nwg partial results of the window, evaluates omega at the two
// extrema and writes the window's entry of the record; the workgroup of window 0 also writes step and closure (the maximum of the
// finite close[y]; -inf when there is none).  Windows beyond the spec's: psi = omega = NaN, cell (-1, -1).
template <typename R, int SEM, bool PROM, bool SHAPE = false>
__global__ __launch_bounds__(BLK) void k_topo_final(const double* __restrict__ partial, int nwg, const double* __restrict__ close, Fields<R, SEM, PROM, SHAPE> f,
                                                   TopoSpec sp, double step, double* __restrict__ rec) {
    __shared__ double sh[BLK / RED_WAVE][TOPO_PART + 1];
    const int i = blockIdx.x, z = blockIdx.y, wave = threadIdx.x / RED_WAVE;
    const Geo& geo = f.geo;
    rec += (size_t)z * TOPO_REC;
    double* out = rec + 2 + 8 * i;   // min {psi, x, y, omega}, max {psi, x, y, omega}
    const bool used = i < sp.nwindows;
    if (!used) {
        if (threadIdx.x < 8) out[threadIdx.x] = (threadIdx.x & 3) == 1 || (threadIdx.x & 3) == 2 ? -1.0 : __builtin_nan("");
        if (i > 0) return;   // (a spec without windows: the workgroup of window 0 still writes step and closure)
    }
    const double* p = partial + ((size_t)z * LBM_TOPOLOGY_MAX_WINDOWS + i) * nwg * TOPO_PART;
    TopoPair e = TopoPair::identity();
    for (int k = threadIdx.x; used && k < nwg; k += BLK) TopoPair::fold(e, red_load<TopoPair>(p + (size_t)k * TOPO_PART));
    double cl = -__builtin_inf();
    if (i == 0) {
        close += (size_t)z * geo.ny;
        for (int y = threadIdx.x; y < geo.ny; y += BLK) {
            const double v = close[y];
            cl = (__builtin_isfinite(v) && v > cl) ? v : cl;
        }
#pragma unroll
        for (int off = RED_WAVE / 2; off > 0; off >>= 1) {
            const double v = __shfl_down(cl, off, RED_WAVE);
            cl = v > cl ? v : cl;
        }
    }
    red_wave(e);
    if (threadIdx.x % RED_WAVE == 0) {
        red_store(sh[wave], e);
        sh[wave][TOPO_PART] = cl;
    }
    __syncthreads();
    if (used && threadIdx.x < 2) {   // thread 0: the minimum, thread 1: the maximum
        const int o = 3 * threadIdx.x;
        TopoCand c{sh[0][o], (int)sh[0][o + 1], (int)sh[0][o + 2]};
        for (int v = 1; v < BLK / RED_WAVE; ++v) {
            const TopoCand b{sh[v][o], (int)sh[v][o + 1], (int)sh[v][o + 2]};
            if (threadIdx.x == 0) topo_fold<false>(c, b); else topo_fold<true>(c, b);
        }
        double* e = out + 4 * threadIdx.x;
        e[0] = c.psi; e[1] = (double)c.x; e[2] = (double)c.y;
        e[3] = c.x >= 0 ? topo_omega_at(f.lattice(z), sp.host_f32, c.x, c.y) : __builtin_nan("");
    }
    if (i == 0 && threadIdx.x == 0) {
        for (int v = 1; v < BLK / RED_WAVE; ++v) cl = sh[v][TOPO_PART] > cl ? sh[v][TOPO_PART] : cl;
        rec[0] = step;
        rec[1] = cl;
    }
}

// omega[z][nx][ny] (host layout) from the staged macroscopic fields of k_export_macro, stage = [z][ux | uy | rho][nx][ny] in the
// lattice's type: every value rounded to host_dtype and widened as the record's are.  One thread per cell, y fastest.
template <typename R>
__global__ __launch_bounds__(BLK) void k_topo_omega(const R* __restrict__ stage, int nx, int ny, int host_f32, double* __restrict__ omega) {
#pragma clang fp contract(off)
    const long long n = (long long)nx * ny, i = (long long)blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    const R* ux = stage + blockIdx.z * 3 * n;
    const R* uy = ux + n;
    const int x = (int)(i / ny), y = (int)(i - (long long)x * ny);
    const double vl = x > 0 ? as_exported(uy[i - ny], host_f32) : 0.0, vr = x < nx - 1 ? as_exported(uy[i + ny], host_f32) : 0.0;
    const double ul = y > 0 ? as_exported(ux[i - 1], host_f32) : 0.0, ur = y < ny - 1 ? as_exported(ux[i + 1], host_f32) : 0.0;
    const double dvdx = topo_diff(vl, as_exported(uy[i], host_f32), vr, x, nx), dudy = topo_diff(ul, as_exported(ux[i], host_f32), ur, y, ny);
    omega[blockIdx.z * n + i] = dvdx + dudy;
}
