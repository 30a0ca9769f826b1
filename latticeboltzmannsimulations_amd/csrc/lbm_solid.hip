// lbm_solid.hip -- liblbm_hip.so: solid obstacles in the bounce-back cavity (lbm_set_solid, lbm_get_solid, lbm_solid_force, and the hold
// cells lbm_set_open_cells, lbm_get_open_cells, the periodic sides lbm_set_periodic, lbm_get_periodic with their kernel k_wrap, and the driving
// force lbm_set_driving_force, lbm_get_driving_force of the C ABI declared in include/lbm.h; LBM_SEM_BOUNCE_BACK_SOLID).  The rule is gather_a<.., SEM_SOLID> (lbm_device.hpp), the step kernel
// k_step_solid (lbm_solid.hpp); here: the mask and the link plane derived from it, the constants of solid cells, and the momentum-
// exchange force (k_solid_force, one template for the three modes of the wall rule) reduced by the tree of lbm_reduce.hpp.  gfx950
// only.  DESIGN.md 2.10.
#include <cmath>

#include "lbm_host.hpp"
#include "lbm_reduce.hpp"

namespace lbmhost {

static_assert(sizeof(lbm_solid_force_record) == 4 * sizeof(double), "record layout");

// Solid cells hold the rest equilibrium at rho = 1, w_k rounded to the lattice type, in both lattices: written after every
// initialisation and upload, from the link plane of `a`.
template <typename R>
__global__ __launch_bounds__(BLK) void k_solid_fix(R* __restrict__ a, R* __restrict__ b, Geo geo, long long bstride) {
    const int x = blockIdx.x * BLK + threadIdx.x, y = blockIdx.y;
    if (x >= geo.nx) return;
    a += blockIdx.z * bstride;
    b += blockIdx.z * bstride;
    const long long me = geo.at(x, y);
    if (!((int)a[K_LINK * geo.plane + me] & LINK_SOLID)) return;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        a[k * geo.plane + me] = weight<R>(k);
        b[k * geo.plane + me] = weight<R>(k);
    }
}

// Hold cells (lbm_set_open_cells) hold their prescribed populations, rounded once to the lattice type, in both lattices: written with the
// constants of the solid cells, from the context's table (OpenTables): one thread per hold cell, cell[i] = (lattice, x, y), val[i][9].
template <typename R>
__global__ __launch_bounds__(BLK) void k_open_fix(R* __restrict__ a, R* __restrict__ b, Geo geo, long long bstride, const int32_t* __restrict__ cell,
                                                  const R* __restrict__ val, int n) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    const long long me = (long long)cell[3 * i] * bstride + geo.at(cell[3 * i + 1], cell[3 * i + 2]);
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        const R v = val[(long long)i * Q + k];
        a[k * geo.plane + me] = v;
        b[k * geo.plane + me] = v;
    }
}

// Periodic sides (lbm_set_periodic): one thread per image cell copies the nine slots of its partner, a real cell, into the image, in the
// lattice a step has just written (or an initialisation, a set_state).  That lattice holds post-collision populations, so the image's
// neighbours then pull what they would pull across the seam.  Thread i: the two image columns first (px: x = 0, then x = nx - 1, y
// running), then the two image rows without the columns' cells (py: y = 0, then y = ny - 1).  A solid image copies the w_k of its solid
// partner.  Plane K_LINK is never copied.  Lattices of a batch on grid axis y.
template <typename R>
__global__ __launch_bounds__(BLK) void k_wrap(R* __restrict__ lat, Geo geo, long long bstride, int px, int py) {
    const int nx = geo.nx, ny = geo.ny;
    const int ncol = px ? 2 * ny : 0, w = px ? nx - 2 : nx, nrow = py ? 2 * w : 0;
    int i = blockIdx.x * BLK + threadIdx.x, x, y;
    if (i >= ncol + nrow) return;
    if (i < ncol) {
        x = i < ny ? 0 : nx - 1;
        y = i < ny ? i : i - ny;
    } else {
        i -= ncol;
        y = i < w ? 0 : ny - 1;
        x = (i < w ? i : i - w) + (px ? 1 : 0);
    }
    const int sx = periodic_partner(x, nx, px != 0), sy = periodic_partner(y, ny, py != 0);
    lat += blockIdx.y * bstride;
    const long long me = geo.at(x, y), from = geo.at(sx, sy);
#pragma unroll
    for (int k = 0; k < Q; ++k) lat[k * geo.plane + me] = lat[k * geo.plane + from];
}

// Momentum exchange: over the (fluid cell, slot k) pairs whose source is a solid cell, links += 1, fx += 2 cx_opp(k) f,
// fy += 2 cy_opp(k) f with f = the cell's post-collision population of direction opp(k) as the lattice holds it, each term converted
// to double.  A lane folds its cells in grid-stride order, slots k = 1 .. 8 in order; then the tree.
struct ForceAcc {
    double links, fx, fy;
    static constexpr int VALS = 3;
    static __device__ __forceinline__ ForceAcc identity() { return ForceAcc{0.0, 0.0, 0.0}; }
    static __device__ __forceinline__ void fold(ForceAcc& a, const ForceAcc& b) {
#pragma clang fp contract(off)
        a.links = a.links + b.links;
        a.fx = a.fx + b.fx;
        a.fy = a.fy + b.fy;
    }
    template <typename F>
    __device__ __forceinline__ void each(F&& f) { f(links); f(fx); f(fy); }
};
constexpr int FORCE_BLOCKS = 256;   // partial results per lattice

// The term of a link by the mode of the wall rule (WallArg), in double without contraction:
//   WALL_REST   f_out = f_in = f:                                         fx += 2 cx_opp(k) f
//   WALL_MOVE   the surface moves, f_out = f - delta:                     fx += cx_opp(k) (2 f - delta), delta as the lattice adds it (the
//               cell's row of the table of lbm_wall_motion.hpp) converted to double
//   WALL_SHAPE  f_out = f (the stores carry no term), f_in = shape_link, what the next gather of the cell returns as slot k:
//                                                                         fx += cx_opp(k) (f_out + f_in), both converted to double
template <typename R, int WALL>
__global__ __launch_bounds__(BLK) void k_solid_force(const R* __restrict__ src, Geo geo, long long bstride, double* __restrict__ partial,
                                                     WallArg<R, WALL> wa) {
#pragma clang fp contract(off)
    __shared__ double shm[BLK / RED_WAVE][ForceAcc::VALS];
    src += blockIdx.z * bstride;
    const long long n = (long long)geo.nx * geo.ny;
    wall_batch(wa, blockIdx.z, geo);
    ForceAcc a = ForceAcc::identity();
    for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < n; i += (long long)gridDim.x * BLK) {
        const int y = (int)(i / geo.nx), x = (int)(i - (long long)y * geo.nx);
        const long long me = geo.at(x, y);
        const int lw = (int)src[K_LINK * geo.plane + me];
        if ((lw & LINK_SOLID) || !(lw & 255)) continue;
        long long row = -1;
        if constexpr (WALL == WALL_MOVE) row = wa.cell_row[i];
        if constexpr (WALL == WALL_SHAPE) row = wa.sh.cell_row[i];
#pragma unroll
        for (int k = 1; k < Q; ++k)
            if ((lw >> (k - 1)) & 1) {
                const R own = src[opp(k) * geo.plane + me];
                a.links = a.links + 1.0;
                if constexpr (WALL == WALL_REST) {
                    const double f = (double)own;
                    a.fx = a.fx + (double)(2 * cxk(opp(k))) * f;
                    a.fy = a.fy + (double)(2 * cyk(opp(k))) * f;
                } else {
                    double t;
                    if constexpr (WALL == WALL_MOVE) t = 2.0 * (double)own - (row >= 0 ? (double)wa.delta[row * 8 + (k - 1)] : 0.0);
                    else t = (double)own + (double)(row >= 0 ? shape_link<R, Geo>(src, geo, wa.sh.ad + row * 16, wa.sh.near[row], k, x, y, own) : own);
                    a.fx = a.fx + (double)cxk(opp(k)) * t;
                    a.fy = a.fy + (double)cyk(opp(k)) * t;
                }
            }
    }
    red_wave(a);
    if (red_workgroup<ForceAcc, BLK / RED_WAVE>(a, shm)) red_store(partial + ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * ForceAcc::VALS, a);
}

// The final pass, one wave per lattice: rec[z] = {step, links, fx, fy}
__global__ __launch_bounds__(RED_WAVE) void k_solid_force_final(const double* __restrict__ partial, int nper, double step, double* __restrict__ rec) {
    const int z = blockIdx.x;
    const ForceAcc a = red_final<ForceAcc>(partial + (size_t)z * nper * ForceAcc::VALS, nper);
    if (threadIdx.x == 0) {
        rec[4 * z] = step;
        red_store(rec + 4 * z + 1, a);
    }
}

template <typename R>
static void wrap_launch(lbm_ctx* c, R* lat, hipStream_t s) {
    const Obstacles& o = c->obs;
    if (!o.periodic()) return;
    const long long n = periodic_images(c->plan.geo.nx, c->plan.geo.ny, o.per_x, o.per_y);
    hipLaunchKernelGGL((k_wrap<R>), dim3((unsigned)((n + BLK - 1) / BLK), c->plan.batch), dim3(BLK), 0, s, lat, c->plan.geo, c->plan.bstride,
                       o.per_x ? 1 : 0, o.per_y ? 1 : 0);
}

int solid_fix(lbm_ctx* c) {
    if (c->p.semantics != LBM_SEM_BOUNCE_BACK_SOLID) return LBM_OK;
    return launch_variant(c, [&](auto v) {
        using R = typename decltype(v)::R;
        hipLaunchKernelGGL((k_solid_fix<R>), grid_rows(c, c->plan.geo.ny), dim3(BLK), 0, c->s_compute, c->lat[0].as<R>(), c->lat[1].as<R>(), c->plan.geo,
                           c->plan.bstride);
        const OpenTables& t = c->obs.open;
        if (t.n > 0)
            hipLaunchKernelGGL((k_open_fix<R>), dim3((t.n + BLK - 1) / BLK), dim3(BLK), 0, c->s_compute, c->lat[0].as<R>(), c->lat[1].as<R>(), c->plan.geo,
                               c->plan.bstride, t.cell, (const R*)t.val, t.n);
        for (int l = 0; l < 2; ++l) wrap_launch<R>(c, c->lat[l].as<R>(), c->s_compute);   // (periodic sides: behind the constants, on both lattices)
    });
}

// The image cells of lat[which] from their partners, on stream s; nothing on a context without periodic sides.
int periodic_wrap(lbm_ctx* c, int which, hipStream_t s) {
    if (!c->obs.periodic()) return LBM_OK;
    return periodic_wrap_lattice(c, c->lat[which].get(), s);
}
// ... of any lattice in the context's layout and type (the scalar lattices: lbm_scalar.hip), by the same launch
int periodic_wrap_lattice(lbm_ctx* c, void* lat, hipStream_t s) {
    if (!c->obs.periodic()) return LBM_OK;
    return launch_variant(c, [&](auto v) { wrap_launch<typename decltype(v)::R>(c, (typename decltype(v)::R*)lat, s); });
}

// Plane K_LINK of lat[0] -> lat[to], all lattices of a batch, on s_compute.  The two lattices get their link planes from lbm_set_solid;
// the lattices that come later -- the scratch lattices of the frame passes, the lattice of the step before the last (multi-step units:
// LBM_FLAG_SOLID_TILES) -- are read by the same gathers, which take the link word from their source, and get a copy when they are
// allocated and at every lbm_set_solid.  Ghost rows and pad columns included (zero in lat[0]).
int solid_copy_links(lbm_ctx* c, int to) {
    if (c->p.semantics != LBM_SEM_BOUNCE_BACK_SOLID || to == 0 || !c->lat[to]) return LBM_OK;
    const Geo& g = c->plan.geo;
    const size_t es = (size_t)c->plan.es, rows = (size_t)g.ny + 2 * GHY;
    const bool by_rows = g.row != g.pitch;   // [y][k][x]: one row of the plane per lattice row; [k][y][x]: the plane is contiguous
    const size_t width = (by_rows ? (size_t)g.pitch : (size_t)g.pitch * rows) * es;
    const size_t pitch = (by_rows ? (size_t)g.row : (size_t)c->plan.bstride) * es;
    const size_t height = by_rows ? rows * c->plan.batch : (size_t)c->plan.batch;
    const size_t off = (size_t)K_LINK * g.plane * es;
    HIP_TRY(c, hipMemcpy2DAsync(c->lat[to].as<char>() + off, pitch, c->lat[0].as<const char>() + off, pitch, width, height, hipMemcpyDeviceToDevice, c->s_compute));
    return LBM_OK;
}

// The link words of one lattice from its mask m[nx][ny] (0 / 1) and its hold cells h[nx][ny] (0 / 1; null: none), as the lattice stores
// them: [ny][nx], x fastest.  A hold cell's word is LINK_HOLD alone.
template <typename R>
static void link_words(const uint8_t* m, const uint8_t* h, int nx, int ny, R* out) {
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            int wd = m[(size_t)x * ny + y] ? LINK_SOLID : 0;
            if (h && h[(size_t)x * ny + y]) {
                out[(size_t)y * nx + x] = (R)LINK_HOLD;
                continue;
            }
            for (int k = 1; k < Q; ++k) {
                const int sx = x - cxk(k), sy = y + cyk(k);
                if (sx >= 0 && sx < nx && sy >= 0 && sy < ny && m[(size_t)sx * ny + sy]) wd |= 1 << (k - 1);
            }
            out[(size_t)y * nx + x] = (R)wd;
        }
}

// mask, hold (null: none): 0 / 1, [batch][nx][ny]
template <typename R>
static int upload_links_as(lbm_ctx* c, const uint8_t* mask, const uint8_t* hold) {
    const Geo& g = c->plan.geo;
    const size_t n = (size_t)g.nx * g.ny;
    std::vector<R> words(n);
    for (int b = 0; b < c->plan.batch; ++b) {
        link_words<R>(mask + (size_t)b * n, hold ? hold + (size_t)b * n : nullptr, g.nx, g.ny, words.data());
        for (int l = 0; l < 2; ++l) {   // plane K_LINK of both lattices: rows of nx words, geo.row elements apart
            R* dst = c->lat[l].as<R>() + (size_t)b * c->plan.bstride + K_LINK * g.plane + g.at(0, 0);
            HIP_TRY(c, hipMemcpy2D(dst, (size_t)g.row * sizeof(R), words.data(), (size_t)g.nx * sizeof(R), (size_t)g.nx * sizeof(R), (size_t)g.ny,
                                   hipMemcpyHostToDevice));
        }
    }
    return LBM_OK;
}

// The link planes of next.mask (lbm_set_solid; no hold cells) or of the context's mask with next.hold (lbm_set_open_cells) into every
// lattice the context holds, before obstacles_change commits it.  A copy that fails part-way leaves the planes of the two lattices in an
// undefined mix of the old and the new: the call returns LBM_ERR_HIP, lbm_get_solid and lbm_get_open_cells still report the old state,
// and the context must be given a mask again (or destroyed) before it steps.
static int upload_links(lbm_ctx* c, const Obstacles& next) {
    const uint8_t* mask = next.mask.empty() ? c->obs.mask.data() : next.mask.data();
    int rc = c->plan.es == 4 ? upload_links_as<float>(c, mask, next.hold_or_null()) : upload_links_as<double>(c, mask, next.hold_or_null());
    for (int i = 2; i < NLAT && rc == LBM_OK; ++i) rc = solid_copy_links(c, i);   // (the lattices allocated since: scratch, the lagged one)
    return rc ? rc : sync_all(c);
}

// The tables of the hold cells (OpenTables): next.hold in the order lattice, x, y, and next.hold_f rounded once to the lattice type.
static int open_tables(lbm_ctx* c, Obstacles& next) {
    if (next.hold.empty()) return LBM_OK;
    const size_t n = (size_t)c->plan.geo.nx * c->plan.geo.ny, ny = (size_t)c->plan.geo.ny;
    std::vector<int32_t> cell;
    for (size_t i = 0; i < next.hold.size(); ++i)
        if (next.hold[i]) {
            cell.push_back((int32_t)(i / n));
            cell.push_back((int32_t)((i % n) / ny));
            cell.push_back((int32_t)(i % ny));
        }
    const bool f32 = c->plan.es == 4;
    std::vector<char> val(next.hold_f.size() * (f32 ? sizeof(float) : sizeof(double)));
    for (size_t i = 0; i < next.hold_f.size(); ++i) {
        if (f32) ((float*)val.data())[i] = (float)next.hold_f[i];
        else ((double*)val.data())[i] = next.hold_f[i];
    }
    if (cell.size() / 3 > 0x7fffffffu) return fail(c, LBM_ERR_INVALID, "lbm_set_open_cells: too many hold cells");
    Pack<HipMem> p = upload<HipMem>({{cell.data(), cell.size() * sizeof(int32_t)}, {val.data(), val.size()}}, "hold cell tables");
    if (!p.err.empty()) return fail(c, p.no_memory ? LBM_ERR_NOMEM : LBM_ERR_HIP, p.err);
    next.open.cell = p.at<const int32_t>(0);
    next.open.val = p.at<const void>(1);
    next.open.n = (int)(cell.size() / 3);
    next.open.base = std::move(p.buf);
    return LBM_OK;
}

// next.per_x, per_y and next.hold_all for the user's hold cells next.hold over the context's mask (lbm_periodic.hpp); a user hold cell on
// an image cell is refused.  Without a periodic side hold_all stays empty.
static int periodic_hold_all(lbm_ctx* c, Obstacles& next, bool px, bool py, const char* call) {
    next.per_x = px;
    next.per_y = py;
    next.hold_all.clear();
    if (!px && !py) return LBM_OK;
    const size_t n = (size_t)c->plan.geo.nx * c->plan.geo.ny, B = (size_t)c->plan.batch;
    next.hold_all.resize(B * n);
    for (size_t b = 0; b < B; ++b) {
        const long long bad = periodic_hold(c->obs.mask.data() + b * n, next.hold.empty() ? nullptr : next.hold.data() + b * n, c->plan.geo.nx, c->plan.geo.ny, px,
                                            py, next.hold_all.data() + b * n);
        if (bad >= 0)
            return fail(c, LBM_ERR_INVALID, std::string(call) + ": lattice " + std::to_string(b) + ": hold cell " + std::to_string(bad) +
                                                " is an image cell of a periodic side (it holds its partner's populations)");
        size_t fluid = 0;
        for (size_t i = 0; i < n; ++i) fluid += !next.hold_all[b * n + i] && !c->obs.mask[b * n + i] ? 1 : 0;
        if (fluid == 0) return fail(c, LBM_ERR_INVALID, std::string(call) + ": lattice " + std::to_string(b) + " is left without a fluid cell");
    }
    return LBM_OK;
}
// One plane of a relaxation field from the caller's [B][nx][ny]: rows as the buoyancy plane's (buoy_at), each value rounded once to the
// lattice type; ghost and pad elements hold `fill`.
template <typename R>
static std::vector<R> relax_plane(const lbm_ctx* c, const double* v, double fill) {
    const Geo& g = c->plan.geo;
    const size_t per = (size_t)buoy_elems(g), n = (size_t)g.nx * g.ny;
    std::vector<R> h(per * c->plan.batch, (R)fill);
    for (int b = 0; b < c->plan.batch; ++b)
        for (int x = 0; x < g.nx; ++x)
            for (int y = 0; y < g.ny; ++y) h[b * per + (size_t)buoy_at(g, x, y)] = (R)v[b * n + (size_t)x * g.ny + y];
    return h;
}
template <typename R>
static int relax_upload(lbm_ctx* c, const double* v, double fill, const char* what, DevBuf* out) {
    const std::vector<R> h = relax_plane<R>(c, v, fill);
    DevBuf d;
    const int rc = alloc_ok(c, d.alloc(h.size() * sizeof(R), what));
    if (rc) return rc;
    HIP_TRY(c, hipMemcpy(d.get(), h.data(), h.size() * sizeof(R), hipMemcpyHostToDevice));
    *out = std::move(d);
    return LBM_OK;
}
template <typename R>
static int relax_download(lbm_ctx* c, const DevBuf& d, double* out) {
    const Geo& g = c->plan.geo;
    const size_t per = (size_t)buoy_elems(g), n = (size_t)g.nx * g.ny;
    std::vector<R> h(per * c->plan.batch);
    HIP_TRY(c, hipMemcpy(h.data(), d.get(), h.size() * sizeof(R), hipMemcpyDeviceToHost));
    for (int b = 0; b < c->plan.batch; ++b)
        for (int x = 0; x < g.nx; ++x)
            for (int y = 0; y < g.ny; ++y) out[b * n + (size_t)x * g.ny + y] = (double)h[b * per + (size_t)buoy_at(g, x, y)];
    return LBM_OK;
}
// The first value that is not finite or not in (0, 2): its index, or -1
static long long relax_bad(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!(std::isfinite(v[i]) && v[i] > 0.0 && v[i] < 2.0)) return (long long)i;
    return -1;
}

}  // namespace lbmhost

using namespace lbmhost;

extern "C" {

int lbm_set_solid(lbm_ctx* c, const uint8_t* mask) {
    if (!c || !mask) return fail(c, LBM_ERR_INVALID, "lbm_set_solid: bad argument");
    int rc = need_solid(c, "lbm_set_solid");
    if (rc) return rc;
    const size_t n = (size_t)c->plan.geo.nx * c->plan.geo.ny;
    for (int b = 0; b < c->plan.batch; ++b) {
        size_t solid = 0;
        for (size_t i = 0; i < n; ++i) solid += mask[(size_t)b * n + i] ? 1 : 0;
        if (solid == n) return fail(c, LBM_ERR_INVALID, "lbm_set_solid: lattice " + std::to_string(b) + " of the mask has no fluid cell");
    }
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    if (rc) return rc;
    // The host copy changes only once both lattices hold the new link planes (upload_links), and one body again, at rest, whatever
    // lbm_set_solid_bodies and lbm_set_body_motion had set.
    Obstacles next;
    next.mask.resize(n * c->plan.batch);
    for (size_t i = 0; i < next.mask.size(); ++i) next.mask[i] = mask[i] ? 1 : 0;
    rc = obstacles_change(c, ObsLevel::mask, next, upload_links);
    if (rc) return rc;
    return lbm_init_equilibrium(c);   // (ends every sampler; solid cells get w_k: solid_fix)
}

int lbm_get_solid(lbm_ctx* c, uint8_t* mask_out) {
    if (!c || !mask_out) return fail(c, LBM_ERR_INVALID, "lbm_get_solid: bad argument");
    const int rc = need_solid(c, "lbm_get_solid");
    if (rc) return rc;
    std::memcpy(mask_out, c->obs.mask.data(), c->obs.mask.size());
    return LBM_OK;
}

int lbm_set_open_cells(lbm_ctx* c, const uint8_t* hold, const double* f) {
    if (!c) return LBM_ERR_INVALID;
    int rc = need_solid(c, "lbm_set_open_cells");
    if (rc) return rc;
    rc = need_one_step(c, "lbm_set_open_cells", "knows no hold cells");
    if (rc) return rc;
    if (!c->obs.shape_q.empty() || c->obs.moves())
        return fail(c, LBM_ERR_STATE, "lbm_set_open_cells: a shape, a body motion or a wall velocity is set (geometry comes first: the hold cells, "
                                      "then lbm_set_solid_shape, lbm_set_body_motion and lbm_set_wall_velocity)");
    const size_t n = (size_t)c->plan.geo.nx * c->plan.geo.ny, B = (size_t)c->plan.batch;
    Obstacles next;
    bool any = false;
    for (size_t i = 0; hold && i < B * n && !any; ++i) any = hold[i] != 0;
    if (any && !f) return fail(c, LBM_ERR_INVALID, "lbm_set_open_cells: hold cells need their populations (f is NULL)");   // (all zero clears, as NULL)
    if (any) {
        next.hold.resize(B * n);
        for (size_t b = 0; b < B; ++b) {
            size_t fluid = 0;
            for (size_t i = 0; i < n; ++i) {
                const bool h = hold[b * n + i] != 0;
                next.hold[b * n + i] = h ? 1 : 0;
                fluid += !h && !c->obs.mask[b * n + i] ? 1 : 0;
                if (!h) continue;
                if (c->obs.mask[b * n + i])
                    return fail(c, LBM_ERR_INVALID, "lbm_set_open_cells: lattice " + std::to_string(b) + ": hold cell " + std::to_string(i) + " is a solid cell");
                for (int k = 0; k < Q; ++k) {
                    const double v = f[(b * Q + k) * n + i];
                    if (!std::isfinite(v) || v < 0.0)
                        return fail(c, LBM_ERR_INVALID, "lbm_set_open_cells: lattice " + std::to_string(b) + ": a population of hold cell " + std::to_string(i) +
                                                            " is not finite or is negative");
                    next.hold_f.push_back(v);
                }
            }
            if (fluid == 0) return fail(c, LBM_ERR_INVALID, "lbm_set_open_cells: lattice " + std::to_string(b) + " is left without a fluid cell");
        }
    }
    rc = periodic_hold_all(c, next, c->obs.per_x, c->obs.per_y, "lbm_set_open_cells");   // (periodic sides stay)
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    if (rc == LBM_OK) rc = open_tables(c, next);
    if (rc == LBM_OK) rc = obstacles_change(c, ObsLevel::open, next, upload_links, "lbm_set_open_cells");
    if (rc) return rc;
    return lbm_init_equilibrium(c);   // (ends every sampler; hold cells get their populations: solid_fix)
}

int lbm_set_periodic(lbm_ctx* c, int px, int py) {
    if (!c) return LBM_ERR_INVALID;
    int rc = need_solid(c, "lbm_set_periodic");
    if (rc) return rc;
    rc = need_one_step(c, "lbm_set_periodic", "knows no image cells");
    if (rc) return rc;
    if (!c->obs.shape_q.empty() || c->obs.moves())
        return fail(c, LBM_ERR_STATE, "lbm_set_periodic: a shape, a body motion or a wall velocity is set (geometry comes first: the periodic sides, "
                                      "then lbm_set_solid_shape, lbm_set_body_motion and lbm_set_wall_velocity)");
    const int nx = c->plan.geo.nx, ny = c->plan.geo.ny;
    const bool x = px != 0, y = py != 0;
    if ((x && nx < 4) || (y && ny < 4)) return fail(c, LBM_ERR_INVALID, "lbm_set_periodic: a periodic direction needs at least 4 cells (two images, two real cells)");
    const size_t n = (size_t)nx * ny;
    for (int b = 0; b < c->plan.batch; ++b) {
        bool lab = false;
        const long long bad = periodic_bad_cell(c->obs.mask.data() + b * n, c->obs.label.data() + b * n, nx, ny, x, y, &lab);
        if (bad >= 0)
            return fail(c, LBM_ERR_INVALID, "lbm_set_periodic: lattice " + std::to_string(b) + ": the " + (lab ? "body label" : "mask") + " of image cell " +
                                                std::to_string(bad) + " differs from its partner's (an image cell is solid where its partner is, in the same body)");
    }
    Obstacles next;
    next.hold = c->obs.hold;
    next.hold_f = c->obs.hold_f;
    rc = periodic_hold_all(c, next, x, y, "lbm_set_periodic");
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    if (rc == LBM_OK) rc = open_tables(c, next);
    if (rc == LBM_OK) rc = obstacles_change(c, ObsLevel::open, next, upload_links, "lbm_set_periodic");
    if (rc) return rc;
    return lbm_init_equilibrium(c);   // (ends every sampler; the image cells get their partners' populations: solid_fix)
}

int lbm_get_periodic(lbm_ctx* c, int* px_out, int* py_out) {
    if (!c) return LBM_ERR_INVALID;
    const int rc = need_solid(c, "lbm_get_periodic");
    if (rc) return rc;
    if (px_out) *px_out = c->obs.per_x ? 1 : 0;
    if (py_out) *py_out = c->obs.per_y ? 1 : 0;
    return LBM_OK;
}

int lbm_set_driving_force(lbm_ctx* c, double fx, double fy) {
    if (!c) return LBM_ERR_INVALID;
    if (!std::isfinite(fx) || !std::isfinite(fy)) return fail(c, LBM_ERR_INVALID, "lbm_set_driving_force: the force is not finite");
    if (fx != 0.0 || fy != 0.0) {
        int rc = need_solid(c, "lbm_set_driving_force");
        if (rc) return rc;
        rc = need_one_step(c, "lbm_set_driving_force", "adds no force");
        if (rc) return rc;
    }
    c->drive[0] = fx;   // (travels by value with every launch: the steps already enqueued keep theirs)
    c->drive[1] = fy;
    return LBM_OK;
}

int lbm_get_driving_force(lbm_ctx* c, double* fx_out, double* fy_out) {
    if (!c) return LBM_ERR_INVALID;
    if (fx_out) *fx_out = c->drive[0];
    if (fy_out) *fy_out = c->drive[1];
    return LBM_OK;
}

int lbm_set_subgrid(lbm_ctx* c, double cs2) {
    if (!c) return LBM_ERR_INVALID;
    if (!std::isfinite(cs2) || cs2 < 0.0) return fail(c, LBM_ERR_INVALID, "lbm_set_subgrid: the constant is negative or not finite");
    if (cs2 != 0.0) {
        int rc = need_solid(c, "lbm_set_subgrid");
        if (rc) return rc;
        rc = need_one_step(c, "lbm_set_subgrid", "has no closure");
        if (rc) return rc;
        if (c->scalar.buoyant)
            return fail(c, LBM_ERR_STATE, "lbm_set_subgrid: buoyancy is set (a buoyant flow with the closure needs an eddy diffusivity for the scalar, "
                                          "which there is none; clear it with lbm_set_buoyancy(c, 0, 0, 0) first)");
        if (c->rheology())
            return fail(c, LBM_ERR_STATE, "lbm_set_subgrid: a rheology table is set (the kernels with the closure read no rheology table: every such "
                                          "pairing is one more set of kernel twins; clear it with lbm_set_rheology(c, NULL, NULL, 0, 0) first)");
    }
    c->subgrid = cs2;   // (travels by value with every launch: the steps already enqueued keep theirs; no history, so the state stays)
    return LBM_OK;
}

int lbm_get_subgrid(lbm_ctx* c, double* cs2_out) {
    if (!c) return LBM_ERR_INVALID;
    if (cs2_out) *cs2_out = c->subgrid;
    return LBM_OK;
}

int lbm_set_relaxation_field(lbm_ctx* c, const double* omega, const double* omegam) {
    if (!c) return LBM_ERR_INVALID;
    if (!omega) {
        if (omegam) return fail(c, LBM_ERR_INVALID, "lbm_set_relaxation_field: omegam without omega (the field is cleared with both NULL)");
        if (!c->relax_field()) return LBM_OK;
        HIP_TRY(c, hipSetDevice(c->p.device));
        const int rc = sync_all(c);   // (the steps enqueued read the planes)
        if (rc) return rc;
        c->relax_w = DevBuf{};
        c->relax_wm = DevBuf{};
        return LBM_OK;
    }
    int rc = need_solid(c, "lbm_set_relaxation_field");
    if (rc) return rc;
    rc = need_one_step(c, "lbm_set_relaxation_field", "reads no rate planes");
    if (rc) return rc;
    if (c->scalar.buoyant)
        return fail(c, LBM_ERR_STATE, "lbm_set_relaxation_field: buoyancy is set (the buoyant kernels read no rate planes: every such pairing is one "
                                      "more set of kernel twins; clear it with lbm_set_buoyancy(c, 0, 0, 0) first)");
    if (c->rheology())
        return fail(c, LBM_ERR_STATE, "lbm_set_relaxation_field: a rheology table is set (the kernels that read rate planes read no rheology table: "
                                      "every such pairing is one more set of kernel twins; clear it with lbm_set_rheology(c, NULL, NULL, 0, 0) first)");
    if (omegam && c->p.collision != LBM_TRT)
        return fail(c, LBM_ERR_STATE, "lbm_set_relaxation_field: omegam is TRT's odd rate and this context's collision is not TRT (pass NULL: MRT's "
                                      "other rates stay the lattice's)");
    const Geo& g = c->plan.geo;
    const size_t n = (size_t)g.nx * g.ny, all = n * c->plan.batch;
    for (const double* v : {omega, omegam}) {
        if (!v) continue;
        const long long bad = relax_bad(v, all);
        if (bad < 0) continue;
        const size_t cell = (size_t)bad % n;
        char val[40];
        std::snprintf(val, sizeof val, "%.17g", v[bad]);
        return fail(c, LBM_ERR_INVALID, std::string("lbm_set_relaxation_field: ") + (v == omega ? "omega" : "omegam") + " of lattice " +
                                            std::to_string((size_t)bad / n) + ", cell (" + std::to_string(cell / g.ny) + ", " + std::to_string(cell % g.ny) +
                                            ") is " + val + ": every rate must be finite and in (0, 2)");
    }
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    if (rc) return rc;
    DevBuf w, wm;
    const bool f32 = c->p.dtype == LBM_F32;
    rc = f32 ? relax_upload<float>(c, omega, c->p.omega, "relaxation field", &w) : relax_upload<double>(c, omega, c->p.omega, "relaxation field", &w);
    if (rc == LBM_OK && omegam)
        rc = f32 ? relax_upload<float>(c, omegam, c->p.omegam, "relaxation field (omegam)", &wm)
                 : relax_upload<double>(c, omegam, c->p.omegam, "relaxation field (omegam)", &wm);
    if (rc) return rc;
    c->relax_w = std::move(w);
    c->relax_wm = std::move(wm);
    return LBM_OK;
}

int lbm_get_relaxation_field(lbm_ctx* c, double* omega_out, double* omegam_out) {
    if (!c) return LBM_ERR_INVALID;
    if (!c->relax_field()) return 0;
    HIP_TRY(c, hipSetDevice(c->p.device));
    const bool f32 = c->p.dtype == LBM_F32;
    int rc = LBM_OK;
    if (omega_out) rc = f32 ? relax_download<float>(c, c->relax_w, omega_out) : relax_download<double>(c, c->relax_w, omega_out);
    if (rc == LBM_OK && omegam_out && c->relax_wm)
        rc = f32 ? relax_download<float>(c, c->relax_wm, omegam_out) : relax_download<double>(c, c->relax_wm, omegam_out);
    return rc ? rc : 1;
}

int lbm_set_rheology(lbm_ctx* c, const double* omega, const double* omegam, int n, double g_max) {
    if (!c) return LBM_ERR_INVALID;
    if (!omega) {
        if (omegam) return fail(c, LBM_ERR_INVALID, "lbm_set_rheology: omegam without omega (the table is cleared with omega NULL)");
        if (!c->rheology()) return LBM_OK;
        HIP_TRY(c, hipSetDevice(c->p.device));
        const int rc = sync_all(c);   // (the steps enqueued read the table)
        if (rc) return rc;
        c->rheo_tab = DevBuf{};
        c->rheo_w.clear();
        c->rheo_wm.clear();
        c->rheo_gmax = 0.0;
        return LBM_OK;
    }
    int rc = need_solid(c, "lbm_set_rheology");
    if (rc) return rc;
    rc = need_one_step(c, "lbm_set_rheology", "reads no rheology table");
    if (rc) return rc;
    const char* const twins = ": every such pairing is one more set of kernel twins; clear it with ";
    if (c->scalar.buoyant)
        return fail(c, LBM_ERR_STATE, std::string("lbm_set_rheology: buoyancy is set (the buoyant kernels read no rheology table") + twins +
                                          "lbm_set_buoyancy(c, 0, 0, 0) first)");
    if (c->subgrid > 0.0)
        return fail(c, LBM_ERR_STATE, std::string("lbm_set_rheology: a sub-grid constant is set (the kernels with the closure read no rheology table") + twins +
                                          "lbm_set_subgrid(c, 0) first)");
    if (c->relax_field())
        return fail(c, LBM_ERR_STATE, std::string("lbm_set_rheology: a relaxation field is set (the kernels that read rate planes read no rheology table") +
                                          twins + "lbm_set_relaxation_field(c, NULL, NULL) first)");
    if (omegam && c->p.collision != LBM_TRT)
        return fail(c, LBM_ERR_STATE, "lbm_set_rheology: omegam is TRT's odd rate and this context's collision is not TRT (pass NULL: MRT's other "
                                      "rates stay the lattice's)");
    if (n < RHEO_MIN_ENTRIES || n > RHEO_MAX_ENTRIES)
        return fail(c, LBM_ERR_INVALID, "lbm_set_rheology: n is " + std::to_string(n) + ": a table has 2 to 65536 entries");
    if (!(std::isfinite(g_max) && g_max > 0.0)) {
        char val[40];
        std::snprintf(val, sizeof val, "%.17g", g_max);
        return fail(c, LBM_ERR_INVALID, std::string("lbm_set_rheology: g_max is ") + val + ": the shear of the last entry must be finite and positive");
    }
    for (const double* v : {omega, omegam}) {
        if (!v) continue;
        const long long bad = relax_bad(v, (size_t)n);
        if (bad < 0) continue;
        char val[40];
        std::snprintf(val, sizeof val, "%.17g", v[bad]);
        return fail(c, LBM_ERR_INVALID, std::string("lbm_set_rheology: ") + (v == omega ? "omega" : "omegam") + " of entry " + std::to_string(bad) + " is " +
                                            val + ": every rate must be finite and in (0, 2)");
    }
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    if (rc) return rc;
    const bool f32 = c->p.dtype == LBM_F32;
    DevBuf tab;
    std::vector<double> w((size_t)n), wm(omegam ? (size_t)n : 0);
    auto upload = [&](const auto& t) -> int {   // t: the table in the lattice type
        const int arc = alloc_ok(c, tab.alloc(t.size() * sizeof(t[0]), "rheology table"));
        if (arc) return arc;
        HIP_TRY(c, hipMemcpy(tab.get(), t.data(), t.size() * sizeof(t[0]), hipMemcpyHostToDevice));
        for (int i = 0; i < n; ++i) {
            w[i] = (double)t[(size_t)i * RHEO_STRIDE];
            if (omegam) wm[i] = (double)t[(size_t)i * RHEO_STRIDE + 2];
        }
        return LBM_OK;
    };
    rc = f32 ? upload(rheology_table<float>(omega, omegam, n)) : upload(rheology_table<double>(omega, omegam, n));
    if (rc) return rc;
    c->rheo_tab = std::move(tab);
    c->rheo_w = std::move(w);
    c->rheo_wm = std::move(wm);
    c->rheo_gmax = g_max;
    return LBM_OK;
}

int lbm_get_rheology(lbm_ctx* c, double* omega_out, double* omegam_out, int* n_out, double* g_max_out) {
    if (!c) return LBM_ERR_INVALID;
    if (!c->rheology()) return 0;
    if (n_out) *n_out = (int)c->rheo_w.size();
    if (g_max_out) *g_max_out = c->rheo_gmax;
    if (omega_out) std::memcpy(omega_out, c->rheo_w.data(), c->rheo_w.size() * sizeof(double));
    if (omegam_out && !c->rheo_wm.empty()) std::memcpy(omegam_out, c->rheo_wm.data(), c->rheo_wm.size() * sizeof(double));
    return 1;
}

int lbm_get_open_cells(lbm_ctx* c, uint8_t* hold_out, double* f_out) {
    if (!c) return LBM_ERR_INVALID;
    const int rc = need_solid(c, "lbm_get_open_cells");
    if (rc) return rc;
    const size_t n = (size_t)c->plan.geo.nx * c->plan.geo.ny, B = (size_t)c->plan.batch;
    const std::vector<uint8_t>& h = c->obs.hold;
    if (hold_out) {
        if (h.empty()) std::memset(hold_out, 0, B * n);
        else std::memcpy(hold_out, h.data(), B * n);
    }
    if (f_out) {
        std::memset(f_out, 0, B * Q * n * sizeof(double));
        size_t at = 0;
        for (size_t i = 0; i < h.size(); ++i)
            if (h[i]) {
                for (int k = 0; k < Q; ++k) f_out[((i / n) * Q + k) * n + i % n] = c->obs.hold_f[at + k];
                at += Q;
            }
    }
    return LBM_OK;
}

int lbm_solid_force(lbm_ctx* c, lbm_solid_force_record* out) {
    if (!c || !out) return fail(c, LBM_ERR_INVALID, "lbm_solid_force: bad argument");
    int rc = need_solid(c, "lbm_solid_force");
    if (rc) return rc;
    if (c->nsteps == 0 || c->raw[c->cur])
        return fail(c, LBM_ERR_STATE, "lbm_solid_force: no step yet (the lattice holds post-collision populations after one)");
    HIP_TRY(c, hipSetDevice(c->p.device));
    rc = sync_all(c);
    if (rc) return rc;
    const int B = c->plan.batch;
    rc = alloc_ok(c, c->obs.force_part.ensure((size_t)B * (FORCE_BLOCKS * ForceAcc::VALS + 4) * sizeof(double), "solid force"));
    if (rc) return rc;
    double* part = c->obs.force_part.as<double>();
    double* rec = part + (size_t)B * FORCE_BLOCKS * ForceAcc::VALS;
    rc = launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        with_wall<VT>(c, [&](auto wa, const double*) {
            hipLaunchKernelGGL((k_solid_force<R, decltype(wa)::MODE>), dim3(FORCE_BLOCKS, 1, B), dim3(BLK), 0, c->s_compute, c->lat[c->cur].as<const R>(),
                               c->plan.geo, c->plan.bstride, part, wa);
        });
        hipLaunchKernelGGL(k_solid_force_final, dim3(B), dim3(RED_WAVE), 0, c->s_compute, (const double*)part, FORCE_BLOCKS, (double)c->nsteps, rec);
    });
    if (rc) return rc;
    return records_to_host(c, rec, (size_t)B * sizeof(lbm_solid_force_record), out);
}
}  // extern "C"
