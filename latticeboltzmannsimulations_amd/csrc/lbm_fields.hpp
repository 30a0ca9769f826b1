// lbm_fields.hpp -- the exported state: what lbm_get_fields would return, as every kernel that reads it sees it.  Fields is the view of
// the lattice the last iteration started from (fields_of, lbm_host.hpp, builds it); the kernels of the field export, of lbm_mean_u and
// of the time statistics follow.  The monitor, the residual and the topology (lbm_monitor.hpp, lbm_residual.hpp, lbm_topology.hpp) read
// through the same view.  Included by the host units (through lbm_host.hpp); the step kernels never see it.
#pragma once
#include "lbm_kernels.hpp"

// A value of the lattice's type as lbm_get_fields(host_dtype) hands it out, in double: rounded to float first where host_dtype is
// LBM_F32.  The one spelling of that rounding (storing through the type itself, as the residual's snapshot does, is the same).
template <typename R>
__device__ __forceinline__ double as_exported(R v, int host_f32) { return host_f32 ? (double)(float)v : (double)v; }

// The view.  src holds post-collision values (+ kept slots + parked wall densities), or plain populations where raw != 0; SEM, PROM:
// those of the context's Variant.  x: column, y: local row.  By value in the kernel arguments.
// SHAPE (SEM_SOLID while lbm_set_solid_shape holds a shape; the default, off, is the view as it always was, member for member): the
// table of the interpolated bounce-back, which the gather then applies on the links -- so every reader sees the rule through this view.
template <typename R, bool SHAPE>
struct FieldsShape {};
template <typename R>
struct FieldsShape<R, true> {
    ShapeTable<R> sh;
};
template <typename R, int SEM, bool PROM, bool SHAPE = false>
struct Fields : FieldsShape<R, SHAPE> {
    static constexpr bool SHAPED = SHAPE;
    const R* src;
    Geo geo;
    int raw;
    R uLB;
    long long bstride;   // elements from one lattice of a batch to the next
    __device__ __forceinline__ Fields lattice(unsigned z) const {
        Fields f = *this;
        f.src = src + z * bstride;
        if constexpr (SHAPE) f.sh.cell_row += (long long)z * geo.nx * geo.ny;
        return f;
    }
    // the populations after streaming and the wall rules (the link plane of a solid mask, the promoted wall equilibrium)
    __device__ __forceinline__ void populations(int x, int y, R (&g)[Q]) const {
        if constexpr (SHAPE) gather_a<R, SEM, Geo, PROM, true>(src, geo, geo, raw, uLB, x, y, g, nullptr, this->sh);
        else gather<R, SEM, PROM>(src, geo, raw, uLB, x, y, g);
    }
    // ... and their moments with the wall overrides, which go by the global row
    __device__ __forceinline__ void macro(int x, int y, R& ux, R& uy, R& rho) const {
        R g[Q];
        populations(x, y, g);
        macros<R, false, SEM>(g, x, geo.y0 + y, geo.nx, geo.NY, uLB, rho, ux, uy);
    }
    __device__ __forceinline__ void exported(int x, int y, int host_f32, double& dux, double& duy, double& drho) const {
        R ux, uy, rho;
        macro(x, y, ux, uy, rho);
        dux = as_exported(ux, host_f32); duy = as_exported(uy, host_f32); drho = as_exported(rho, host_f32);
    }
};

// lattice -> staging: current populations (post stream + wall rules) in host layout
template <typename R, int SEM, bool PROM, bool SHAPE = false>
__global__ __launch_bounds__(BLK) void k_export_fin(Fields<R, SEM, PROM, SHAPE> f, R* __restrict__ stage) {
    const Geo& geo = f.geo;
    constexpr int TRX = trx<R>(), RY = BLK / TRX;
    __shared__ R t[Q][TRX][33];
    const long long n = (long long)geo.nx * geo.ny;
    const auto lat = f.lattice(blockIdx.z);
    stage += blockIdx.z * (Q * n);
    const int x0 = blockIdx.x * TRX, y0 = blockIdx.y * 32;
    const int tx = threadIdx.x % TRX, x = x0 + tx;
    for (int ty = threadIdx.x / TRX; ty < 32; ty += RY) {   // gather along x
        const int y = y0 + ty;
        if (x >= geo.nx || y >= geo.ny) continue;
        R g[Q];
        lat.populations(x, y, g);
#pragma unroll
        for (int k = 0; k < Q; ++k) t[k][tx][ty] = g[k];
    }
    __syncthreads();
    const int yy = threadIdx.x & 31, xb = threadIdx.x >> 5;
    for (int xx = xb; xx < TRX; xx += BLK / 32)              // write along y
        if (x0 + xx < geo.nx && y0 + yy < geo.ny) {
#pragma unroll
            for (int k = 0; k < Q; ++k) stage[k * n + (long long)(x0 + xx) * geo.ny + y0 + yy] = t[k][xx][yy];
        }
}

// lattice -> staging: the macroscopic fields of the view (with wall overrides; SEM_BB: none); stage = [ux | uy | rho], each
// [nx][ny_local]
template <typename R, int SEM, bool PROM, bool SHAPE = false>
__global__ __launch_bounds__(BLK) void k_export_macro(Fields<R, SEM, PROM, SHAPE> f, R* __restrict__ stage) {
    const Geo& geo = f.geo;
    constexpr int TRX = trx<R>(), RY = BLK / TRX;
    __shared__ R t[3][TRX][33];
    const long long n = (long long)geo.nx * geo.ny;
    const auto lat = f.lattice(blockIdx.z);
    stage += blockIdx.z * (3 * n);
    const int x0 = blockIdx.x * TRX, y0 = blockIdx.y * 32;
    const int tx = threadIdx.x % TRX, x = x0 + tx;
    for (int ty = threadIdx.x / TRX; ty < 32; ty += RY) {
        const int y = y0 + ty;
        if (x >= geo.nx || y >= geo.ny) continue;
        R rho, ux, uy;
        lat.macro(x, y, ux, uy, rho);
        t[0][tx][ty] = ux; t[1][tx][ty] = uy; t[2][tx][ty] = rho;
    }
    __syncthreads();
    const int yy = threadIdx.x & 31, xb = threadIdx.x >> 5;
    for (int xx = xb; xx < TRX; xx += BLK / 32)
        if (x0 + xx < geo.nx && y0 + yy < geo.ny) {
            const long long o = (long long)(x0 + xx) * geo.ny + y0 + yy;
            stage[o] = t[0][xx][yy];
            stage[n + o] = t[1][xx][yy];
            stage[2 * n + o] = t[2][xx][yy];
        }
}

// lattice -> staging: relaxation time tau + tau_turbulent of the iteration that starts from the populations of the view (taus_g,
// MRT_GPU.py:385-387; the closure runs in MRT_GPU.py semantics only); turb = 0: the constant 1 / omega.  stage = [nx][ny_local]
template <typename R, bool FAST, bool PROM>
__global__ __launch_bounds__(BLK) void k_export_tau(Fields<R, SEM_GPU, PROM> f, Relax<R> w, Batch<R> bt, int turb, R* __restrict__ stage) {
    const Geo& geo = f.geo;
    constexpr int TRX = trx<R>(), RY = BLK / TRX;
    __shared__ R t[TRX][33];
    const long long n = (long long)geo.nx * geo.ny;
    const auto lat = f.lattice(blockIdx.z);
    if (bt.w) w = bt.w[blockIdx.z];
    stage += blockIdx.z * n;
    const int x0 = blockIdx.x * TRX, y0 = blockIdx.y * 32;
    const int tx = threadIdx.x % TRX, x = x0 + tx;
    for (int ty = threadIdx.x / TRX; ty < 32; ty += RY) {
        const int y = y0 + ty;
        if (x >= geo.nx || y >= geo.ny) continue;
        R tau = (R)1.0 / w.w_nu;
        if (turb) {
            R g[Q];
            lat.populations(x, y, g);
            const long long me = geo.at(x, y);
            tau = smagorinsky_tau<R, FAST, PROM>(g, lat.src[K_QEQ * geo.plane + me], lat.src[K_RHO * geo.plane + me], w.w_nu);
        }
        t[tx][ty] = tau;
    }
    __syncthreads();
    const int yy = threadIdx.x & 31, xb = threadIdx.x >> 5;
    for (int xx = xb; xx < TRX; xx += BLK / 32)
        if (x0 + xx < geo.nx && y0 + yy < geo.ny) stage[(long long)(x0 + xx) * geo.ny + y0 + yy] = t[xx][yy];
}

// ... of an obstacle lattice with the sub-grid closure (lbm_set_subgrid): the tau that the step from the view's lattice gives each cell --
// subgrid_tau of the populations the view gathers under the context's wall rule and of their moments, the operations of the step
// (FAST: its divisions and square roots); a solid cell and a hold cell, which no step updates, report tau0.  k: sgs_k.  stage = [nx][ny_local]
template <typename R, bool FAST, bool SHAPE>
__global__ __launch_bounds__(BLK) void k_export_tau_subgrid(Fields<R, SEM_SOLID, false, SHAPE> f, Relax<R> w, Batch<R> bt, R k, R* __restrict__ stage) {
    const Geo& geo = f.geo;
    constexpr int TRX = trx<R>(), RY = BLK / TRX;
    __shared__ R t[TRX][33];
    const long long n = (long long)geo.nx * geo.ny;
    const auto lat = f.lattice(blockIdx.z);
    if (bt.w) w = bt.w[blockIdx.z];
    stage += blockIdx.z * n;
    const int x0 = blockIdx.x * TRX, y0 = blockIdx.y * 32;
    const int tx = threadIdx.x % TRX, x = x0 + tx;
    for (int ty = threadIdx.x / TRX; ty < 32; ty += RY) {
        const int y = y0 + ty;
        if (x >= geo.nx || y >= geo.ny) continue;
        R tau = (R)1.0 / w.w_nu;
        if (!((int)lat.src[K_LINK * geo.plane + geo.at(x, y)] & (LINK_SOLID | LINK_HOLD))) {
            R g[Q], rho, ux, uy;
            lat.populations(x, y, g);
            macros<R, FAST, SEM_SOLID>(g, x, geo.y0 + y, geo.nx, geo.NY, lat.uLB, rho, ux, uy);
            tau = subgrid_tau<R, FAST>(g, rho, ux, uy, w.w_nu, k);
        }
        t[tx][ty] = tau;
    }
    __syncthreads();
    const int yy = threadIdx.x & 31, xb = threadIdx.x >> 5;
    for (int xx = xb; xx < TRX; xx += BLK / 32)
        if (x0 + xx < geo.nx && y0 + yy < geo.ny) stage[(long long)(x0 + xx) * geo.ny + y0 + yy] = t[xx][yy];
}

// ... with a relaxation field (lbm_set_relaxation_field; rw: the plane of the cells' viscous rates, buoy_at): a cell that is neither solid
// nor held reports 1 / rw of the cell in the lattice type or, SGS (the closure with k), subgrid_tau on that rate; the others tau0.
template <typename R, bool FAST, bool SHAPE, bool SGS>
__global__ __launch_bounds__(BLK) void k_export_tau_relax(Fields<R, SEM_SOLID, false, SHAPE> f, Relax<R> w, Batch<R> bt, R k, const R* __restrict__ rw,
                                                          R* __restrict__ stage) {
    const Geo& geo = f.geo;
    constexpr int TRX = trx<R>(), RY = BLK / TRX;
    __shared__ R t[TRX][33];
    const long long n = (long long)geo.nx * geo.ny;
    const auto lat = f.lattice(blockIdx.z);
    if (bt.w) w = bt.w[blockIdx.z];
    stage += blockIdx.z * n;
    rw += blockIdx.z * buoy_elems(geo);
    const int x0 = blockIdx.x * TRX, y0 = blockIdx.y * 32;
    const int tx = threadIdx.x % TRX, x = x0 + tx;
    for (int ty = threadIdx.x / TRX; ty < 32; ty += RY) {
        const int y = y0 + ty;
        if (x >= geo.nx || y >= geo.ny) continue;
        R tau = (R)1.0 / w.w_nu;
        if (!((int)lat.src[K_LINK * geo.plane + geo.at(x, y)] & (LINK_SOLID | LINK_HOLD))) {
            const R wc = rw[buoy_at(geo, x, y)];
            if constexpr (SGS) {
                R g[Q], rho, ux, uy;
                lat.populations(x, y, g);
                macros<R, FAST, SEM_SOLID>(g, x, geo.y0 + y, geo.nx, geo.NY, lat.uLB, rho, ux, uy);
                tau = subgrid_tau<R, FAST>(g, rho, ux, uy, wc, k);
            } else {
                tau = (R)1.0 / wc;
            }
        }
        t[tx][ty] = tau;
    }
    __syncthreads();
    const int yy = threadIdx.x & 31, xb = threadIdx.x >> 5;
    for (int xx = xb; xx < TRX; xx += BLK / 32)
        if (x0 + xx < geo.nx && y0 + yy < geo.ny) stage[(long long)(x0 + xx) * geo.ny + y0 + yy] = t[xx][yy];
}

// ... with a rheology table (lbm_set_rheology; rh: the context's table, lbm_device.hpp), and the shear itself (lbm_get_shear), two outputs of
// which either may be null: a cell that is neither solid nor held reports, in tau, 1 / w_nu of rheology_rates on the populations the view
// gathers and their moments -- the operations of the step (FAST: its division, square root and fused interpolation), then one division in
// the lattice type -- and, in shear, g = N / rho of rheology_shear; a solid cell and a hold cell report tau0 and 0.  tau needs a table
// (rh.tab), shear does not.  tau, shear = [nx][ny_local] per lattice.
template <typename R, bool FAST, bool SHAPE>
__global__ __launch_bounds__(BLK) void k_export_rheology(Fields<R, SEM_SOLID, false, SHAPE> f, Relax<R> w, Batch<R> bt, Rheo<R> rh, R* __restrict__ tau,
                                                         R* __restrict__ shear) {
    const Geo& geo = f.geo;
    constexpr int TRX = trx<R>(), RY = BLK / TRX;
    __shared__ R t[2][TRX][33];
    const long long n = (long long)geo.nx * geo.ny;
    const auto lat = f.lattice(blockIdx.z);
    if (bt.w) w = bt.w[blockIdx.z];
    const int x0 = blockIdx.x * TRX, y0 = blockIdx.y * 32;
    const int tx = threadIdx.x % TRX, x = x0 + tx;
    for (int ty = threadIdx.x / TRX; ty < 32; ty += RY) {
        const int y = y0 + ty;
        if (x >= geo.nx || y >= geo.ny) continue;
        R tc = (R)1.0 / w.w_nu, gc = (R)0;
        if (!((int)lat.src[K_LINK * geo.plane + geo.at(x, y)] & (LINK_SOLID | LINK_HOLD))) {
            R g[Q], rho, ux, uy;
            lat.populations(x, y, g);
            macros<R, FAST, SEM_SOLID>(g, x, geo.y0 + y, geo.nx, geo.NY, lat.uLB, rho, ux, uy);
            gc = rheology_shear<R, FAST>(g, rho, ux, uy);
            if (tau) {
                R w_nu, w_m;
                rheology_rates<R, FAST>(g, rho, ux, uy, rh, w.w_m, w_nu, w_m);
                tc = div_<FAST>((R)1.0, w_nu);
            }
        }
        t[0][tx][ty] = tc;
        t[1][tx][ty] = gc;
    }
    __syncthreads();
    const int yy = threadIdx.x & 31, xb = threadIdx.x >> 5;
    for (int xx = xb; xx < TRX; xx += BLK / 32)
        if (x0 + xx < geo.nx && y0 + yy < geo.ny) {
            const long long o = blockIdx.z * n + (long long)(x0 + xx) * geo.ny + y0 + yy;
            if (tau) tau[o] = t[0][xx][yy];
            if (shear) shear[o] = t[1][xx][yy];
        }
}

// Sum over the slab of ux + uy of the view's macroscopic state (what k_export_macro would write), in double:
// partial[blockIdx.z * gridDim.x + blockIdx.x] = the block's sum; k_reduce_final adds the partial sums of each lattice in
// index order -- a fixed summation tree, so the result does not vary from run to run.
template <typename R, int SEM, bool PROM, bool SHAPE = false>
__global__ __launch_bounds__(BLK) void k_reduce_u(Fields<R, SEM, PROM, SHAPE> f, double* __restrict__ partial) {
    __shared__ double red[BLK];
    const Geo& geo = f.geo;
    const auto lat = f.lattice(blockIdx.z);
    const long long n = (long long)geo.nx * geo.ny;
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < n; i += (long long)gridDim.x * BLK) {
        const int y = (int)(i / geo.nx), x = (int)(i - (long long)y * geo.nx);
        R rho, ux, uy;
        lat.macro(x, y, ux, uy, rho);
        acc += (double)ux + (double)uy;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = BLK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)blockIdx.z * gridDim.x + blockIdx.x] = red[0];
}

// Time statistics (lbm_stats_*): per cell, the macroscopic state k_export_macro would export (the same view, so the same bits),
// converted to double and added to six running sums acc = [S_u | S_v | S_rho | S_uu | S_vv | S_uv], each plane
// [ny_local][nxa], x fastest (nxa = nx rounded up to even; lattice b of a batch at acc + b * 6 * ny_local * nxa; the padding column
// stays 0).  One lane owns the two neighbouring cells 2i, 2i + 1 of the flattened plane: every access to the sums is 16 B per lane and
// coalesced along x.  Contraction off: each product is rounded in double, then added -- the same operations, in the same order, as
// the host loop  acc += u.astype(f64); acc2 += u64 * u64  over lbm_get_fields.  One thread owns a cell: no atomics, samples add in
// the order they are enqueued.  Pure streaming: 9 * sizeof(R) + 48 B read and 48 B written per cell.
template <typename R, int SEM, bool PROM, bool SHAPE = false>
__global__ __launch_bounds__(BLK) void k_stats_accumulate(Fields<R, SEM, PROM, SHAPE> f, double* __restrict__ acc) {
#pragma clang fp contract(off)
    typedef double d2 __attribute__((ext_vector_type(2)));
    const Geo& geo = f.geo;
    const int nxh = (geo.nx + 1) >> 1;
    const long long npairs = (long long)geo.ny * nxh;   // = half the elements of one plane
    const auto lat = f.lattice(blockIdx.z);
    d2* a = (d2*)acc + blockIdx.z * 6 * npairs;
    for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < npairs; i += (long long)gridDim.x * BLK) {
        const int y = (int)(i / nxh), x = 2 * (int)(i - (long long)y * nxh);
        d2 u = {0.0, 0.0}, v = {0.0, 0.0}, r = {0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (x + j >= geo.nx) break;   // (the padding column of an odd nx)
            R rho, ux, uy;
            lat.macro(x + j, y, ux, uy, rho);
            u[j] = (double)ux; v[j] = (double)uy; r[j] = (double)rho;
        }
        a[i] = a[i] + u;
        a[npairs + i] = a[npairs + i] + v;
        a[2 * npairs + i] = a[2 * npairs + i] + r;
        a[3 * npairs + i] = a[3 * npairs + i] + u * u;
        a[4 * npairs + i] = a[4 * npairs + i] + v * v;
        a[5 * npairs + i] = a[5 * npairs + i] + u * v;
    }
}
